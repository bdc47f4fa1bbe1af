"""Inputs shared by tests/test_policy_host.py (CPU) and tests/test_gpu_policy.py: the two networks,
their weights, the feature batches, and the stock fp32 forward that E_bf16 is measured against.
Everything here runs on the CPU (torch + the C oracle)."""
from __future__ import annotations

import functools

import numpy as np

SEED = 0x5EED
BATCHES = (1, 63, 64, 65, 127, 128, 257)
NET_REF = (449, 128, 150, 128, 5)   # actor_critic.Policy on the default options
NET_ODD = (37, 17, 40, 9, 6)        # nothing a multiple of the tile; the 6-action option set
NET_WIDE = (50, 200, 256, 130, 5)   # h1 > 128: two layer-1 tiles per wave; a width at the 256 limit
OPTS_REF = {"max_turns": 5}
OPTS_ODD = {"max_turns": 5, "gatherer_only": False, "lookout_only": False}
WARM_STEPS = 7                       # steps before the features are taken (max_turns = 5: two episodes)


def make_state_dict(net, seed, scaled="affine2", scale=3.0):
    """torch's default Linear init under a fixed seed, one layer's weights and bias scaled x3.
    Two units of the third layer get a bias that drives them to the clamp limits whatever the
    input: -500 (leaky_relu gives -5, clamped to -4: a default init never reaches -400) and +10
    (clamped to +4); every other unit is as initialised."""
    import torch

    F, h1, h2, h3, A = net
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (n_out, n_in) in (("affine1", (h1, F)), ("affine2", (h2, h1)), ("affine3", (h3, h2)),
                                ("action_head", (A, h3)), ("value_head", (1, h3))):
        bound = 1.0 / np.sqrt(n_in)  # kaiming_uniform(a=sqrt(5)) on the weight, the same bound on the bias
        k = scale if name == scaled else 1.0
        sd[name + ".weight"] = ((torch.rand((n_out, n_in), generator=g) * 2 - 1) * bound * k).float()
        sd[name + ".bias"] = ((torch.rand((n_out,), generator=g) * 2 - 1) * bound * k).float()
    sd["affine3.bias"][0] = -500.0
    if h3 > 1:
        sd["affine3.bias"][1] = 10.0
    return sd


@functools.lru_cache(maxsize=None)
def weights(which, variant=0):
    net = {"ref": NET_REF, "odd": NET_ODD, "wide": NET_WIDE}[which]
    return make_state_dict(net, 1234 + 17 * variant + {"ref": 0, "odd": 5, "wide": 9}[which])


def fp32_forward(sd, features):
    """actor_critic.Policy.forward in stock torch fp32 on the CPU, weights not rounded."""
    import torch
    import torch.nn.functional as Fn

    x = torch.as_tensor(features).float()
    x = Fn.leaky_relu(Fn.linear(x, sd["affine1.weight"], sd["affine1.bias"]))
    x = Fn.leaky_relu(Fn.linear(x, sd["affine2.weight"], sd["affine2.bias"]))
    x = Fn.leaky_relu(Fn.linear(x, sd["affine3.weight"], sd["affine3.bias"]))
    x = torch.clamp(x, -4, 4)
    probs = Fn.softmax(Fn.linear(x, sd["action_head.weight"], sd["action_head.bias"]), dim=-1)
    return probs, Fn.linear(x, sd["value_head.weight"], sd["value_head.bias"])[:, 0]


def contract_cost(sd, features):
    """E_bf16 of these inputs: max |reference_forward - stock fp32 forward| for probs and value."""
    from wab_gym_amd.policy import reference_forward

    rp, rv = reference_forward(sd, features)
    fp, fv = fp32_forward(sd, features)
    return float((rp - fp.double()).abs().max()), float((rv - fv.double()).abs().max())


def warm_actions(B, n_actions, steps=WARM_STEPS):
    """The pre-chosen actions of the warm-up steps, [steps, B]."""
    return np.random.RandomState(100 + B).randint(n_actions, size=(steps, B)).astype(np.int8)


def oracle_after_warmup(B, opts=None, env_id_base=0):
    """A C-oracle batch (options OPTS_REF unless given) reset and stepped through warm_actions."""
    from oracle.oracle import OracleBatch

    orc = OracleBatch(dict(OPTS_REF if opts is None else opts), B, SEED, env_id_base)
    orc.reset()
    for a in warm_actions(B, orc.n_actions):
        orc.step(a)
    return orc


def oracle_features(orc):
    from oracle.oracle import featurize

    vm = np.zeros((orc.B, 11, 11), np.uint8)
    return featurize(orc.planes, orc.food_turns, orc.role, orc.status, vm, orc.W, orc.H,
                     orc.options["turns_to_empty_food"])


@functools.lru_cache(maxsize=None)
def ref_features(B):
    """Real features [B, 449] of the default options after the warm-up (from the C oracle; the GPU
    test asserts that wab_step_features gives the same)."""
    return oracle_features(oracle_after_warmup(B))


@functools.lru_cache(maxsize=None)
def odd_features(B, F=37):
    """A hand-made [B, F] batch (F >= 37): 0/1 entries, multiples of 1/8, and a few floats that
    bf16 cannot hold."""
    rng = np.random.RandomState(7 + B + F)
    x = rng.randint(2, size=(B, F)).astype(np.float32)
    x[:, 10:20] = rng.randint(-16, 17, size=(B, 10)) / 8.0
    x[:, 30:34] = rng.standard_normal((B, 4)).astype(np.float32)
    x[:, 36] = np.float32(1.0) / np.float32(3.0)
    return x


# ------------------------------------------------------------------ nets whose fp32 sums are exact
# (F, h1, h2, h3, A) of tests/test_gpu_policy.py's exact-arithmetic cases -> what
# wab_debug_policy_plan must say of it: (input chunks of layer 1, columns per chunk KC, the last
# chunk's columns, LDS bytes, 1 for wab_policy_kernel<true>).  A is 5 or 6, the only action counts
# a handle can have.  Both instances run at 1, 2, 3 and 4 chunks.
EXACT_SHAPES = {
    (1, 1, 1, 1, 5): (1, 16, 16, 20480, 0),             # the minimum of everything; the d.F - 1 column clamp
    (16, 32, 32, 32, 6): (1, 16, 16, 20480, 0),         # exact tile multiples
    (17, 33, 33, 33, 5): (1, 32, 32, 36864, 0),         # one past the tile in every dimension
    (1000, 8, 8, 8, 6): (4, 256, 240, 77824, 0),        # KC clamped to 256
    (449, 128, 150, 128, 5): (3, 160, 144, 77824, 0),   # NT1 = 4: the widest <false>
    (449, 129, 150, 128, 6): (3, 160, 144, 86016, 1),   # NT1 = 5: waves 1-3 have no second tile
    (449, 256, 256, 256, 5): (2, 240, 224, 135168, 1),  # one workgroup per CU; the budget < x2 branch
    (560, 130, 8, 8, 5): (4, 144, 128, 81920, 1),       # <true> at 4 chunks
    (16, 130, 8, 8, 6): (1, 16, 16, 53248, 1),          # <true> at 1 chunk
    (300, 32, 32, 32, 5): (2, 160, 144, 53248, 0),      # <false> at 2 chunks
}
EXACT_BATCHES = (1, 127, 128, 129, 257)  # a workgroup takes 128 envs


@functools.lru_cache(maxsize=None)
def exact_features(B, F):
    """[B, F] features that are 0 / 1 or, every third column from column 0, multiples of 1/8 in
    [0, 2]: exact in bf16 and never negative (exact_net's units rely on the sign)."""
    rng = np.random.RandomState(31 + B + 7 * F)
    x = rng.randint(2, size=(B, F)).astype(np.float32)
    x[:, ::3] = rng.randint(0, 17, size=x[:, ::3].shape) / 8.0
    return x


def exact_net(shape, seed=0):
    """A state dict whose forward pass the kernel must reproduce without rounding in any sum
    (exact_certificate checks that it does, from the reference alone).

    Weights and biases are small dyadic numbers, a few nonzeros per unit, and every input
    column and every unit of every layer has at least one nonzero weight.  What keeps the sums
    exact is that no hidden value is both tiny and finely grained: the features are never
    negative and each hidden unit's pre-activation has one sign on all inputs.  Even units
    ("plus") have a bias >= 0, weights > 0 on plus inputs and < 0 on minus inputs; odd units
    ("minus") the opposite with a bias <= -1/2, so 0.01 * z never compounds into 1e-4 * z.  In
    the third layer unit 0 has bias 16 (clamped to 4) and unit 1 bias -448 (leaky_relu gives
    -4.48, clamped to -4) whatever the input.  The all-ones net, whose single units must take
    both signs, is written out by hand: z1 = 2 f - 1, z2 = 2 x1 - 1, z3 = 16 - 128 x2."""
    import torch

    F, h1, h2, h3, A = shape
    rng = np.random.RandomState(4000 + seed)
    sd = {}

    def put(name, w, b):
        sd[name + ".weight"] = torch.tensor(w, dtype=torch.float32)
        sd[name + ".bias"] = torch.tensor(b, dtype=torch.float32)

    def cover(w, mags, sign_of):
        """a nonzero weight in every column that has none, spread over the units in turn"""
        n_out = w.shape[0]
        for k in np.nonzero(~w.any(axis=0))[0]:
            n = int(k) % n_out
            w[n, k] = sign_of(n, k) * rng.choice(mags)

    if (h1, h2, h3) == (1, 1, 1):
        if F != 1:
            raise ValueError("exact_net: a net of single units is written for F = 1")
        put("affine1", [[2.0]], [-1.0])
        put("affine2", [[2.0]], [-1.0])
        put("affine3", [[-128.0]], [16.0])
    elif min(h1, h2, h3) < 2:
        raise ValueError("exact_net: hidden layers need a plus and a minus unit (width >= 2)")
    else:
        in_sign = np.ones(F)
        for i, (name, n_out, n_in) in enumerate((("affine1", h1, F), ("affine2", h2, h1), ("affine3", h3, h2))):
            unit_sign = np.where(np.arange(n_out) % 2 == 0, 1.0, -1.0)
            mags = (0.5, 1.0, 2.0) if i == 0 else (1.0, 2.0)
            w = np.zeros((n_out, n_in))
            for n in range(n_out):
                for k in rng.choice(n_in, size=min(n_in, 3 if i == 0 else 2), replace=False):
                    w[n, k] = unit_sign[n] * in_sign[k] * rng.choice(mags)
            cover(w, mags[:1], lambda n, k: unit_sign[n] * in_sign[k])
            if i < 2:
                b = np.where(unit_sign > 0, rng.choice((0.0, 0.5, 1.0), size=n_out), rng.choice((-0.5, -1.0), size=n_out))
            else:  # both kinds of unit end coarse: plus >= 1/2, minus <= -0.32 after the slope
                b = np.where(unit_sign > 0, rng.choice((0.5, 1.0), size=n_out), rng.choice((-32.0, -64.0), size=n_out))
                b[0], b[1] = 16.0, -448.0
                w[1] *= 32.0
            put(name, w, b)
            in_sign = unit_sign
    head_mags = (0.25, 0.5, 1.0)
    wa = np.zeros((A, h3))
    for n in range(A):
        for k in rng.choice(h3, size=min(h3, 3), replace=False):
            wa[n, k] = rng.choice((-1.0, 1.0)) * rng.choice(head_mags)
    cover(wa, head_mags[:1], lambda n, k: rng.choice((-1.0, 1.0)))
    put("action_head", wa, rng.choice((-0.5, 0.0, 0.25, 1.0), size=A))
    put("value_head", rng.choice((-1.0, 1.0), size=(1, h3)) * rng.choice(head_mags[:2], size=(1, h3)), [0.5])
    return sd


def _low_bit_exponent(v):
    """e with 2^e the lowest set bit of each float64 in v (a large number where v == 0)."""
    m, e = np.frexp(np.abs(v))
    mant = (m * 2.0 ** 53).astype(np.int64)
    low = np.where(mant != 0, mant & -mant, 1)
    return np.where(mant != 0, e - 53 + np.round(np.log2(low.astype(np.float64))).astype(np.int64), 1 << 20)


def exact_certificate(sd, features):
    """Asserts, from reference_forward alone, that the kernel has nothing to round on these inputs
    but expf and the softmax's divide; returns the smallest headroom found, in bits.

    1. For every matmul, unit and env: with 2^q the largest power of two that divides every
       bf16 x bf16 term and the bias, sum |terms| + |bias| < 2^24 * 2^q.  Every partial sum, in
       any order and with the bias added last, is then a multiple of 2^q below 2^(q + 24): a
       float32, exactly.  (headroom = q + 24 - log2 of that sum.)
    2. bias, leaky_relu, clamp and the bf16 rounding done in float32, as the kernel does them,
       give the bf16 values of reference_forward's float64 step."""
    import torch

    from wab_gym_amd.policy import LAYERS, reference_forward

    def bf(x):
        return torch.as_tensor(x).to(torch.float32).to(torch.bfloat16).to(torch.float64)

    hidden = []
    reference_forward(sd, features, hidden=hidden)
    x = bf(features).numpy()
    headroom = np.inf
    for i, name in enumerate(LAYERS):
        w = bf(sd[name + ".weight"]).numpy()
        b = sd[name + ".bias"].to(torch.float64).numpy()
        lx, lw = _low_bit_exponent(x), _low_bit_exponent(w)
        total = np.abs(x) @ np.abs(w).T + np.abs(b)[None, :]
        q = np.broadcast_to(_low_bit_exponent(b)[None, :], total.shape).copy()
        for n in range(w.shape[0]):
            nz = np.nonzero(w[n])[0]
            if len(nz):
                q[:, n] = np.minimum(q[:, n], (lx[:, nz] + lw[n, nz][None, :]).min(axis=1))
        live = total > 0
        assert (q[live] < (1 << 19)).all()
        room = q[live] + 24 - np.log2(total[live])
        assert (room > 0).all(), (name, float(room.min()))
        headroom = min(headroom, float(room.min())) if live.any() else headroom
        if i < 3:
            z, out = hidden[i]
            z32 = z.to(torch.float32)
            assert torch.equal(z32.to(torch.float64), z), name  # (follows from 1.)
            y = torch.where(z32 >= 0, z32, torch.tensor(0.01, dtype=torch.float32) * z32)
            if i == 2:
                y = y.clamp(-4.0, 4.0)
            assert y.dtype == torch.float32 and torch.equal(y.to(torch.bfloat16).to(torch.float64), out), name
            x = out.numpy()
    return headroom
