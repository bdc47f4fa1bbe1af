"""wab_policy_grad on the GPU where a slab holds more than one row block.

wab_policy_wgrad_kernel gives row block b (128 rows) to slab b % S and folds a slab's blocks in
ascending order into fp32 accumulators that live in the workspace between chunks; S depends on
the net alone (tests/policy_grad_cases.py SLABS), so below 128 S rows (5248 to 8192) no slab
folds twice and tests/test_gpu_policy_grad.py never gets there.  Every N here is built from S:

1. the fold order inside a slab, bit for bit: one live row per block in blocks 0, S, 2 S, 1,
   S + 1, 5 and the last; the result is predicted from single-row runs on the CPU and differs
   from the descending and the slab-less orders.  Inside a slab the sum is the MFMA's own
   accumulate, which is not fl32(acc + term): pgc.mfma_accumulate models it, and
   tests/test_policy_grad_host.py holds the model to the instruction's recorded results.
   Measured: of the seven-row sums, 9 (odd), 172 (ref), 8 ((449,129,150,128,6)) and 0
   ((17,33,33,33,5)) elements differ from the fold by float32 adds, each by one unit in the
   last place;
2. chunk_rows changes no bit when chunks start at and past block S, at multiples of S, and when
   the default chunk of 32768 rows is crossed;
3. every tensor, loss and row output within half of E with two or more blocks in every slab;
4. nothing is left behind: a smaller call and an empty call after a large one on the same
   workspace, and the bad-action count over several chunks.

Measured on an MI355X (max |kernel - contract| / E, worst case per tensor): see DESIGN.md,
"wab_policy_grad.hip"."""
import ctypes

import numpy as np
import pytest
import torch

import policy_grad_cases as pgc
import test_gpu_policy_grad as tg
from wab_gym_amd import _lib, policy

pytestmark = pytest.mark.gpu
LOSSES = ("loss_policy", "loss_value", "entropy", "loss")
ROW_OUTPUTS = ("logp", "value", "entropy_rows")


def slabs_of(pol, net):
    """S as the library plans it; pinned to the table."""
    plan = (ctypes.c_int32 * 5)()
    _lib.check(_lib.load().wab_debug_policy_grad_plan(pol._p, 0, plan), "wab_debug_policy_grad_plan")
    assert plan[0] == pgc.GRAD_ROWS and plan[2] == 32768
    assert plan[1] == pgc.SLABS[net] == pgc.plan_slabs(net), (net, plan[1])
    return int(plan[1])


def f32(t):
    return t.numpy().astype(np.float32, copy=False)


def same_bits(got, want):
    return tuple(got.shape) == tuple(want.shape) and torch.equal(got, torch.as_tensor(want))


def first_difference(r1, r2):
    """The first output of two runs that differs, or None: the ten tensors, the four losses and
    the three row outputs."""
    for k in pgc.GRAD_NAMES:
        if not tg.same(r1["grads"][k], r2["grads"][k]):
            return k
    for k in LOSSES + ROW_OUTPUTS:
        if not tg.same(r1[k], r2[k]):
            return k
    return None


# ------------------------------------------------------------------ 1. the fold order inside a slab
@pytest.mark.parametrize("net", ((17, 33, 33, 33, 5), (449, 129, 150, 128, 6), "odd", "ref"), ids=str)
def test_a_slab_folds_its_blocks_in_ascending_order(net):
    pol = tg.policy_for(net)
    S = slabs_of(pol, net)
    n = pgc.fold_rows_n(S)
    assert (n + 127) // 128 == 2 * S + 3 and n % 128 == 5
    x = pgc.features(net, n)
    a, w, t = pgc.rows(net, n)
    value = tg.run(pol, x, a, w, t)["value"].numpy()
    live = pgc.fold_live_rows(S)
    assert live[-1][1] == n - 1 and [b % S for b, _ in live] == [0, 0, 0, 1, 1, 5, 2]

    # the terms: one live row each.  Every other row has G_4 = 0 exactly, so an output element gets
    # one nonzero bf16 x bf16 product, exact in fp32, and 0 + term = term in every sum
    runs = {b: tg.run(pol, x, a, *tg.one_live(w, t, value, (i,))) for b, i in live}
    terms = {k: {b: f32(runs[b]["grads"][k]) for b, _ in live} for k in pgc.GRAD_NAMES}
    xs = tg.layer_inputs(net, x) if isinstance(net, tuple) else None
    x0 = torch.as_tensor(x).to(torch.bfloat16).float().numpy()
    factors = {k: {} for k in pgc.GRAD_NAMES}  # the term of block b is a * b, bf16 values: db_l and [x_{l-1} | 1]
    for b, i in live:
        assert float(runs[b]["loss_policy"]) != 0.0 and float(runs[b]["loss_value"]) != 0.0, (b, i)
        for layer in policy.LAYERS:
            db, dW = terms[layer + ".bias"][b], terms[layer + ".weight"][b]
            assert bool(db.any()), (layer, b, i)
            u = int(np.argmax(np.abs(db)))
            xl = (dW[u].astype(np.float64) / float(db[u])).astype(np.float32)
            # the term itself at rows past block S: dW_l the outer product of db_l and x_{l-1}
            assert np.array_equal(db.astype(np.float64)[:, None] * xl.astype(np.float64)[None, :], dW), (layer, b, i)
            assert np.array_equal(torch.as_tensor(db).to(torch.bfloat16).float().numpy(), db), (layer, b, i)
            if layer == "affine1":
                assert np.array_equal(xl, x0[i]), (b, i)
            if xs is not None:
                assert np.array_equal(xl.astype(np.float64), xs[layer][i].numpy()), (layer, b, i)
            factors[layer + ".weight"][b] = (db[:, None], xl[None, :])
            factors[layer + ".bias"][b] = (db, np.float32(1.0))

    def predicted(k, order="slabs", scale=1.0, blocks=None):
        """The slabs' sums as the MFMA accumulates them (pgc.mfma_accumulate), added in float32."""
        use = {b: terms[k][b] for b in (blocks or terms[k])}
        return pgc.fold(use, S, order, scale, factors=factors[k])

    # two rows of one slab, blocks 0 and S: the accumulator after block 0 is its term, then one MFMA.
    # (fl32(term_0 + term_S) it is not, in about one element of 200 of those that round:
    # tools/micro/mfma_accumulate.hip)
    two = tg.run(pol, x, a, *tg.one_live(w, t, value, (live[0][1], live[1][1])))
    for k in pgc.GRAD_NAMES:
        assert same_bits(two["grads"][k], predicted(k, blocks=(0, S))), k

    # all seven: slabs ascending of (the slab's blocks ascending), times scale; in one chunk, and
    # in chunks of three blocks (the accumulators go through the workspace between a slab's blocks)
    w7, t7 = tg.one_live(w, t, value, [i for _, i in live])
    ieee = 0
    for scale, chunk_rows in ((1.0, 0), (0.25, 0), (1.0, 128 * 3)):
        got = tg.run(pol, x, a, w7, t7, scale=scale, chunk_rows=chunk_rows)
        for k in pgc.GRAD_NAMES:
            assert same_bits(got["grads"][k], predicted(k, "slabs", scale)), (k, scale, chunk_rows)
            if (scale, chunk_rows) == (1.0, 0):
                ieee += int((f32(got["grads"][k]) != pgc.fold(terms[k], S, "slabs")).sum())
        for k in ("loss_policy", "loss_value"):  # the parts are returned unscaled
            want = np.float32(pgc.fold_f64({b: float(runs[b][k]) for b, _ in live}, S))
            assert f32(got[k]) == want, (k, scale, float(got[k]), float(want))
            assert want == np.float32(sum(float(runs[b][k]) for b, _ in live)), k
    print("%s: %d elements of the seven-row sum are not the fold by float32 adds" % (net, ieee))

    # non-vacuity: the other orders give other bits (the exact nets may have sums without an order)
    for order in ("descending", "flat"):
        differ = [k for k in pgc.GRAD_NAMES if k.endswith(".weight")
                  and not np.array_equal(predicted(k, order), predicted(k))]
        print("%s: the %s fold differs from the kernel's order in %s" % (net, order, differ))
        if not isinstance(net, tuple):
            assert differ, order
    pol.close()


# ------------------------------------------------------------------ 2. chunking at and past S
@pytest.mark.parametrize("net", ("ref", (17, 33, 33, 33, 5)), ids=str)
def test_chunks_that_start_at_and_past_block_S_change_no_bit(net):
    pol = tg.policy_for(net)
    S = slabs_of(pol, net)
    n = pgc.fold_rows_n(S)
    x = pgc.features(net, n)
    a, w, t = pgc.rows(net, n)
    kw = dict(value_coef=0.5, entropy_coef=0.01)
    base = tg.run(pol, x, a, w, t, **kw)  # one chunk
    assert all(bool((base["grads"][k] != 0).any()) for k in pgc.GRAD_NAMES)
    # one block per chunk; B0 through every residue and past S; every chunk from a multiple of S; B0 = S + 1
    for chunk_rows in (128, 128 * 3, 128 * S, 128 * (S + 1)):
        got = tg.run(pol, x, a, w, t, chunk_rows=chunk_rows, **kw)
        assert first_difference(base, got) is None, (chunk_rows, first_difference(base, got))
    assert first_difference(base, tg.run(pol, x, a, w, t, **kw)) is None
    pol.close()


def test_crossing_the_default_chunk_changes_no_bit():
    net = (17, 33, 33, 33, 5)
    pol = tg.policy_for(net)
    slabs_of(pol, net)
    n = 32768 + 129
    x = pgc.features(net, n)
    a, w, t = pgc.rows(net, n)
    kw = dict(value_coef=0.5, entropy_coef=0.01)
    two_chunks = tg.run(pol, x, a, w, t, **kw)
    one_chunk = tg.run(pol, x, a, w, t, chunk_rows=65536, **kw)
    assert first_difference(two_chunks, one_chunk) is None, first_difference(two_chunks, one_chunk)
    ref, E = pgc.contract_and_cost(net, n, 0.5, 0.01)
    tg.check_gate(two_chunks, ref, E, "%s N=%d two chunks" % (net, n))
    pol.close()


# ------------------------------------------------------------------ 3. against the contract, two blocks per slab
@pytest.mark.parametrize("net", ("ref", "odd", "wide", (449, 129, 150, 128, 6)), ids=str)
def test_against_the_contract_with_two_blocks_in_every_slab(net):
    pol = tg.policy_for(net)
    S = slabs_of(pol, net)
    n = pgc.two_per_slab_n(S)
    assert (n + 127) // 128 == 2 * S + 2
    x = pgc.features(net, n)
    a, w, t = pgc.rows(net, n)
    worst, failed = {}, []
    for value_loss in ("smooth_l1", "mse"):
        for ec in (0.0, 0.01):
            ref, E = pgc.contract_and_cost(net, n, 0.5, ec, value_loss)
            got = tg.run(pol, x, a, w, t, value_coef=0.5, entropy_coef=ec, value_loss=value_loss)
            try:
                tg.check_gate(got, ref, E, "%s N=%d %s ec=%g" % (net, n, value_loss, ec), worst)
            except AssertionError as e:  # (every ratio is printed before the test fails)
                failed.append(e)
    print("worst ratios, %s N=%d: %s" % (net, n, "  ".join("%s %.4f" % kv for kv in sorted(worst.items()))))
    assert not failed, failed
    pol.close()


# ------------------------------------------------------------------ 4. state left behind
def test_a_smaller_call_on_the_same_workspace_is_a_fresh_one():
    pol = tg.policy_for("ref")
    S = slabs_of(pol, "ref")
    kw = dict(value_coef=0.5, entropy_coef=0.01)
    n = pgc.two_per_slab_n(S)
    big = tg.run(pol, pgc.features("ref", n), *pgc.rows("ref", n), **kw)  # every slab, row and loss partial used
    assert all(bool((big["grads"][k] != 0).any()) for k in pgc.GRAD_NAMES)
    empty = (np.zeros((0, 449), np.float32), np.zeros(0, np.int8), np.zeros(0, np.float32), np.zeros(0, np.float32))
    for n, args in ((130, (pgc.features("ref", 130),) + pgc.rows("ref", 130)), (0, empty)):
        used = tg.run(pol, *args, **kw)
        fresh = tg.policy_for("ref")
        want = tg.run(fresh, *args, **kw)
        fresh.close()
        assert first_difference(want, used) is None, (n, first_difference(want, used))
        assert all(bool((used["grads"][k] != 0).any()) == (n > 0) for k in pgc.GRAD_NAMES), n
    assert all(float(used[k]) == 0.0 for k in LOSSES)
    pol.close()


def test_bad_actions_are_counted_over_blocks_and_chunks():
    pol = tg.policy_for("ref")
    S = slabs_of(pol, "ref")
    n = pgc.two_per_slab_n(S)
    x = pgc.features("ref", n)
    a, w, t = pgc.rows("ref", n)
    args = [tg.dev(x, torch.float32), None, tg.dev(w, torch.float32), tg.dev(t, torch.float32)]
    clean = pol.loss_and_grad(args[0], tg.dev(a, torch.int8), *args[2:], return_rows=True)
    pol.check()
    value = clean["value"].cpu().numpy()
    # block S + 1; with chunks of three blocks, the second chunk (blocks 3..5) and the last (the last row)
    def weighted_row_of(block):
        return block * 128 + int(np.nonzero(w[block * 128:(block + 1) * 128])[0][-1])

    bad_rows = (weighted_row_of(S + 1), weighted_row_of(4), n - 1)
    blocks = (n + 127) // 128
    assert bad_rows[0] // 128 == S + 1 and bad_rows[1] // (128 * 3) == 1 and (n - 1) // (128 * 3) == (blocks - 1) // 3
    a_bad, a_ok, w_ok, t_ok = a.copy(), a.copy(), w.copy(), t.copy()
    for i, action in zip(bad_rows, (5, -1, 127)):
        a_bad[i] = action
        w_ok[i] = 0.0
        t_ok[i] = value[i]
    want = pol.loss_and_grad(args[0], tg.dev(a_ok, torch.int8), tg.dev(w_ok, torch.float32),
                             tg.dev(t_ok, torch.float32))
    pol.check()
    assert not tg.same(want["grads"]["affine1.weight"], clean["grads"]["affine1.weight"])
    for chunk_rows in (0, 128 * 3):
        got = pol.loss_and_grad(args[0], tg.dev(a_bad, torch.int8), *args[2:], chunk_rows=chunk_rows)
        with pytest.raises(IndexError, match=r"wab_policy_grad: 3 rows had"):
            pol.check()
        for k in pgc.GRAD_NAMES:
            assert tg.same(got["grads"][k], want["grads"][k]), (k, chunk_rows)
        for k in ("loss_policy", "loss_value"):
            assert tg.same(got[k], want[k]), (k, chunk_rows)
        # a following clean call reports none
        again = pol.loss_and_grad(args[0], tg.dev(a, torch.int8), *args[2:], chunk_rows=chunk_rows)
        pol.check()
        assert tg.same(again["loss"], clean["loss"])
    pol.close()
