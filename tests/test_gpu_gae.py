"""wab_gae and wab_whiten on the device.

wab_gae against the numpy contract of tests/gae_cases.py, advantage and target bit for bit (a
NaN standing for any NaN: the payload of an inf - inf is the hardware's), on the segments of
tests/returns_cases.py with a value column.  Each case first asserts the instance the launch
takes, through wab_debug_gae_plan (the host function the launch itself calls).

Which case launches which instance (VEC, NE):
  test_chunk_edges           (1, 0) h = NULL and (1, 3) the defaults, T = 1 .. 129
  test_gamma_lambda_grid     (1, 3)
  test_option_sets           (1, n) at B = 1000 and (2, n) at B = 131072, n = 0, 1, 2, 3, 4, 8 (twice)
  test_vec_dispatch          (2, 3) at B = 131072 aligned, (1, 3) at every layout that must fall back
test_case_lists_cover_every_instance asserts that these name all 12.

wab_whiten against the exact-sum reference within one float32 step, run twice for equal bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gae_cases as gc
import returns_cases as rc
from wab_gym_amd import _lib
from wab_gym_amd.env import BatchedWolvesAndBushesEnv
from wab_gym_amd.wrappers import discounted_returns, gae, whitened

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA, LAM = 0.99, 0.95


@functools.lru_cache(maxsize=None)
def table_env(name):
    """A 64-env handle of the option set: it only supplies the reward table."""
    return BatchedWolvesAndBushesEnv(rc.options_of(name), num_envs=64, seed=1, device=DEV)


@functools.lru_cache(maxsize=2)
def case(T, B, name="defaults"):
    return gc.make_gae_case(T, B, name)


@functools.lru_cache(maxsize=4)
def reference(T, B, name, table, with_last, gamma=GAMMA, lam=LAM):
    reward, done, value, last, opts = case(T, B, name)
    return gc.gae_reference(gc.exact_rewards(reward, opts, table), done, value, last if with_last else None,
                            gamma, lam)


def device_view(host, offset=0):
    """`host` on the device, `offset` elements into a larger (256-byte aligned) buffer."""
    buf = torch.empty(host.size + 8, dtype=torch.from_numpy(host[:0]).dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + host.size].view(host.shape)
    view.copy_(torch.from_numpy(host))
    return view


def plan_of(env, r, d, v, adv, tgt):
    got = (ctypes.c_int32 * 2)(-1, -1)
    _lib.check(_lib.load().wab_debug_gae_plan(None if env is None else env._h, r.data_ptr(), d.data_ptr(),
                                              v.data_ptr(), None if adv is None else adv.data_ptr(),
                                              None if tgt is None else tgt.data_ptr(), r.shape[1], got),
               "wab_debug_gae_plan")
    return got[0], got[1]


def assert_same(got, want, what):
    got = got.cpu().numpy()
    if not gc.same_bits(got, want):
        bad = np.argwhere((gc.bits(got) != gc.bits(want)) & ~(np.isnan(got) & np.isnan(want)))
        raise AssertionError("%s: %d differ, first at (t, b) = %s" % (what, len(bad), bad[:1].tolist()))


def run(name, T, B, table, with_last, want_plan, offsets=(0, 0, 0, 0, 0), gamma=GAMMA, lam=LAM):
    """One gae() call on device copies laid `offsets` elements (reward, done, value, advantage,
    target) into their buffers, against the contract."""
    reward, done, value, last, _ = case(T, B, name)
    env = table_env(name) if table else None
    r, d, v = device_view(reward, offsets[0]), device_view(done, offsets[1]), device_view(value, offsets[2])
    adv = device_view(np.zeros((T, B), np.float32), offsets[3])
    tgt = device_view(np.zeros((T, B), np.float32), offsets[4])
    assert plan_of(env, r, d, v, adv, tgt) == want_plan
    lv = torch.as_tensor(last, device=DEV) if with_last else None
    got = gae(r, d, v, lv, gamma, lam, env=env, advantage=adv, target=tgt)
    assert got[0] is adv and got[1] is tgt
    want = reference(T, B, name, table, with_last, gamma, lam)
    assert_same(adv, want[0], "advantage")
    assert_same(tgt, want[1], "target")


# (B, (reward, done, value, advantage, target) offsets in elements, planned VEC)
DISPATCH = [
    (131072, (0, 0, 0, 0, 0), 2),
    (131072, (1, 0, 0, 0, 0), 1),   # reward 4 bytes in
    (131072, (0, 1, 0, 0, 0), 1),   # done 1 byte in
    (131072, (0, 0, 1, 0, 0), 1),   # value 4 bytes in
    (131072, (0, 0, 0, 1, 0), 1),   # advantage 4 bytes in
    (131072, (0, 0, 0, 0, 1), 1),   # target 4 bytes in
    (131072, (2, 2, 2, 2, 2), 2),   # all 8 (done 2) bytes in: still aligned
    (131073, (0, 0, 0, 0, 0), 1),   # B odd
    (131070, (0, 0, 0, 0, 0), 1),   # B / 2 < 65536
]
NE_BATCHES = ((1000, 1), (131072, 2))
EDGE_T = (1, 31, 32, 33, 64, 65, 129)
EDGE_B = (1, 63, 64, 65, 1000)
GRID = (0.0, 0.95, 0.99, 1.0)


def test_case_lists_cover_every_instance():
    planned = {(vec, 3) for _, _, vec in DISPATCH}
    planned |= {(vec, ne) for _, _, ne in rc.OPTION_SETS for _, vec in NE_BATCHES}
    planned |= {(1, 0), (1, 3)}
    assert planned == {(vec, ne) for vec in (1, 2) for ne in (0, 1, 2, 3, 4, 8)}


@pytest.mark.parametrize("T", EDGE_T)
def test_chunk_edges(T):
    """The 32-step chunks' edges: one chunk short, exact and one step over, two chunks exact and
    one step over, four chunks and a step; one thread, a wave short, exact and one over, several
    workgroups; h = NULL and the default table, last_value given and NULL."""
    for B in EDGE_B:
        for with_last in (True, False):
            run("defaults", T, B, False, with_last, (1, 0))
            run("defaults", T, B, True, with_last, (1, 3))


def test_gamma_lambda_grid():
    for gamma in GRID:
        for lam in GRID:
            run("defaults", 65, 1000, True, True, (1, 3), gamma=gamma, lam=lam)


@pytest.mark.parametrize("B,vec", NE_BATCHES)
@pytest.mark.parametrize("name,ne", [(n, ne) for n, _, ne in rc.OPTION_SETS])
def test_option_sets(name, ne, B, vec):
    """Every reward-table size through a handle, and the same floats with h = NULL."""
    run(name, 33, B, True, True, (vec, ne))
    run(name, 33, B, False, True, (vec, 0))


@pytest.mark.parametrize("B,offsets,vec", DISPATCH)
def test_vec_dispatch(B, offsets, vec):
    """The float2 rows and the 16-bit done load with its byte select at the smallest batch that
    reaches them, and every layout that must fall back to one env per thread; T = 33: two chunks
    with a one-step last chunk."""
    run("defaults", 33, B, True, True, (vec, 3), offsets)


@pytest.mark.parametrize("B", [1000, 131072])
def test_one_output_alone(B):
    reward, done, value, last, _ = case(33, B)
    env = table_env("defaults")
    r, d, v = device_view(reward), device_view(done), device_view(value)
    lv = torch.as_tensor(last, device=DEV)
    want = reference(33, B, "defaults", True, True)
    L = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k, what in enumerate(("advantage", "target")):
        out = torch.full((33, B), float("nan"), device=DEV)
        ptrs = [None, None]
        ptrs[k] = out.data_ptr()
        assert plan_of(env, r, d, v, out if k == 0 else None, out if k == 1 else None) == (2 if B > 1000 else 1, 3)
        _lib.check(L.wab_gae(env._h, r.data_ptr(), d.data_ptr(), v.data_ptr(), lv.data_ptr(), 33, B, GAMMA, LAM,
                             ptrs[0], ptrs[1], stream), "wab_gae")
        assert_same(out, want[k], what + " alone")


def test_done_bytes_and_forced_columns():
    """What make_case builds is what ran: all three nonzero bytes, a never-done and an always-done
    column, the forced dones, and a column of infinities whose NaN stops at the next done."""
    reward, done, value, last, _ = case(65, 1000)
    assert set(np.unique(done).tolist()) == {0, 1, 0x80, 0xFF}
    assert not done[:, 0].any() and done[:, 1].all() and done[0, 2] and done[64, 3] and done[31, 4] and done[32, 5]
    adv, _ = reference(65, 1000, "defaults", True, True)
    assert np.isnan(adv[:, 6]).any() and not np.isnan(adv[:, 6]).all() and np.isfinite(adv[:, :6]).all()
    run("defaults", 65, 1000, True, True, (1, 3))


@pytest.mark.parametrize("T,scale,gamma", [(129, 4.0, 0.99), (129, 1.0e4, 0.99), (65, 4.0, 1.0)])
def test_lambda_one_against_the_returns_kernel(T, scale, gamma):
    """lambda = 1: the targets are the bootstrapped returns of discounted_returns(env=,
    bootstrap=), the existing kernel, within one float32 ulp of the column's largest magnitude
    (identity 3 of tests/test_gae_host.py, the same bound)."""
    B = 1000
    reward, done, value, last, opts = gc.make_gae_case(T, B, scale=scale)
    env = table_env("defaults")
    r, d, v = device_view(reward), device_view(done), device_view(value)
    lv = torch.as_tensor(last, device=DEV)
    _, tgt = gae(r, d, v, lv, gamma, 1.0, env=env)
    R = discounted_returns(r, d, gamma, bootstrap=lv, env=env).cpu().numpy()
    cols = gc.finite_columns(value, last)
    differ, worst = gc.check_lambda_one(tgt.cpu().numpy(), R, np.abs(R).max(0), value, last, cols)
    print("lambda = 1 on the device, T = %d, scale %g, gamma %g: %.4f %% differ, worst %.3g of the bound"
          % (T, scale, gamma, 100 * differ, worst))


def test_refusals():
    T, B = 8, 64
    L = _lib.load()
    r = torch.zeros(T, B, device=DEV)
    v = torch.zeros(T + 1, B, device=DEV)
    d = torch.zeros(T, B, dtype=torch.uint8, device=DEV)
    lv = torch.zeros(B, device=DEV)
    o = torch.zeros(2 * T, B, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    env = table_env("defaults")

    def call(adv, tgt, T=T, h=env._h, reward=r.data_ptr(), value=v.data_ptr()):
        return L.wab_gae(h, reward, d.data_ptr(), value, lv.data_ptr(), T, B, GAMMA, LAM, adv, tgt, s)

    assert call(o.data_ptr(), o[T:].data_ptr()) == 0
    assert call(None, None) == -1                                   # both outputs NULL
    assert call(o.data_ptr(), None, T=-1) == -1
    assert call(v.data_ptr(), None) == -1                           # advantage is value
    assert call(None, v[1:].data_ptr()) == -1                       # target over value, one row in
    assert call(r.data_ptr(), o.data_ptr()) == -1                   # advantage is reward
    assert call(o.data_ptr(), lv.data_ptr()) == -1                  # target starts at last_value
    assert call(d.data_ptr(), None) == -1                           # advantage over done
    assert call(o.data_ptr(), o[T - 1:].data_ptr()) == -1           # the two outputs overlap by a row
    assert b"overlap" in L.wab_last_error()
    assert call(o.data_ptr(), None, reward=None) == -1
    assert call(o.data_ptr(), None, value=None) == -1
    assert call(o.data_ptr(), None, T=0) == 0
    # the wrapper refuses an output that is an input too
    with pytest.raises(ValueError):
        gae(r, d, v[:T], lv, advantage=r)
    # a handle whose table is ambiguous: the C call refuses, the wrapper warns and uses the floats
    amb = BatchedWolvesAndBushesEnv({"reward_for_eating": 2.0 ** -30, "reward_per_turn": 1.0}, num_envs=64, seed=1,
                                    device=DEV)
    assert call(o.data_ptr(), None, h=amb._h) == -1
    assert b"round to the same" in L.wab_last_error()
    got = (ctypes.c_int32 * 2)()
    assert L.wab_debug_gae_plan(amb._h, r.data_ptr(), d.data_ptr(), v.data_ptr(), o.data_ptr(), None, B, got) == -1
    reward, done, value, last, _ = case(33, 64)
    dr, dd, dv = device_view(reward), device_view(done), device_view(value)
    with pytest.warns(UserWarning, match="round to the same"):
        adv, tgt = gae(dr, dd, dv, torch.as_tensor(last, device=DEV), env=amb)
    want = reference(33, 64, "defaults", False, True)
    assert_same(adv, want[0], "advantage")
    assert_same(tgt, want[1], "target")


# ------------------------------------------------------------------ wab_whiten
WHITEN_N = (1, 2, 63, 64, 65, 64 * 1000 + 1, 64 * 65536)


@functools.lru_cache(maxsize=None)
def whiten_case(n):
    x = gc.make_whiten_input(n)
    return x, gc.whiten_reference(x)


def check_whitened(got, want):
    """|out - ref| <= 2^-23 max(1, |ref|); at most 0.1 % of the entries differ at all."""
    got = got.cpu().numpy().astype(np.float64)
    ref = want.astype(np.float64)
    err = np.abs(got - ref)
    assert (err <= 2.0 ** -23 * np.maximum(1.0, np.abs(ref))).all(), float(err.max())
    differ = float((got != ref).mean())
    assert differ <= 1e-3, differ
    return differ


@pytest.mark.parametrize("n", WHITEN_N)
def test_whitened(n):
    x, want = whiten_case(n)
    xd = torch.as_tensor(x, device=DEV)
    got = whitened(xd)
    again = whitened(xd)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))   # two runs, the same bits
    if n == 1:
        assert np.isnan(want).all() and torch.isnan(got).all()
        return
    assert torch.equal(xd.cpu(), torch.from_numpy(x))                  # out of place: x untouched
    differ = check_whitened(got, want)
    print("whitened n = %d: %.2e of the entries differ from the exact-sum reference" % (n, differ))
    y = xd.clone()
    assert whitened(y, out=y) is y
    assert torch.equal(y.view(torch.int32), got.view(torch.int32))       # in place, the same bits
    if n % 64 == 0:
        shaped = whitened(xd.view(64, -1))
        assert shaped.shape == (64, n // 64) and torch.equal(shaped.view(-1), got)


def test_whitened_other_eps_and_unaligned_views():
    x, _ = whiten_case(64 * 1000 + 1)
    xd = torch.as_tensor(x, device=DEV)
    check_whitened(whitened(xd, eps=0.5), gc.whiten_reference(x, 0.5))
    check_whitened(whitened(xd[1:]), gc.whiten_reference(x[1:]))         # 4 bytes off alignment
    L = _lib.load()
    assert L.wab_whiten_workspace(-1) == -1 and L.wab_whiten_workspace((1 << 40) + 1) == -1
    assert L.wab_whiten_workspace(0) == L.wab_whiten_workspace(1 << 40) > 0
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(L.wab_whiten_workspace(8) // 8, dtype=torch.float64, device=DEV)
    assert L.wab_whiten(xd.data_ptr(), 8, 1e-7, xd[4:].data_ptr(), ws.data_ptr(), s) == -1   # partial overlap
    assert L.wab_whiten(xd.data_ptr(), 8, 1e-7, xd.data_ptr(), None, s) == -1
    assert L.wab_whiten(xd.data_ptr(), -1, 1e-7, xd.data_ptr(), ws.data_ptr(), s) == -1
    assert L.wab_whiten(None, 0, 1e-7, None, None, s) == 0


def test_graph_of_gae_and_whitened_replays_to_the_eager_result():
    T, B = 33, 1000
    reward, done, value, last, _ = case(T, B)
    env = table_env("defaults")
    r, d, v = device_view(reward), device_view(done), device_view(value)
    # (the whitening needs finite advantages: the column of infinities becomes a plain one)
    v[:, 6] = v[:, 8]
    lv = torch.as_tensor(last, device=DEV)
    adv, tgt = gae(r, d, v, lv, GAMMA, LAM, env=env)
    white = whitened(adv)
    torch.cuda.synchronize()
    g_adv, g_tgt, g_white = torch.zeros_like(adv), torch.zeros_like(tgt), torch.zeros_like(white)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gae(r, d, v, lv, GAMMA, LAM, env=env, advantage=g_adv, target=g_tgt)
        whitened(g_adv, out=g_white)
    for _ in range(2):
        g_adv.zero_(), g_tgt.zero_(), g_white.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in ((g_adv, adv), (g_tgt, tgt), (g_white, white)):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.isfinite(white).all()
