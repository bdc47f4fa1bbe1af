"""Inputs shared by tests/test_policy_host.py (CPU) and tests/test_gpu_policy.py: the two networks,
their weights, the feature batches, and the stock fp32 forward that E_bf16 is measured against.
Everything here runs on the CPU (torch + the C oracle)."""
from __future__ import annotations

import functools

import numpy as np

SEED = 0x5EED
BATCHES = (1, 63, 64, 65, 257)
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
