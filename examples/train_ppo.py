"""PPO on the device: train_actor_critic.py's loop with K epochs of M minibatches over each rollout
segment.  Per update: one closed-loop rollout with GAE advantages, whitened (wab_rollout_policy,
wab_gae, wab_whiten), one evaluate pass for old_logp (wab_policy_evaluate; old_value is the
rollout's value), then K x M passes of the clipped loss and its gradients (wab_policy_grad_ppo)
over contiguous row ranges features[t0:t1] of the [T, B, F] segment, each followed by
DeviceAdam.step() (wab_policy_adam_step).  With --shuffle every epoch draws a fresh permutation of
the segment's T B rows on the device and minibatch m is its slice perm[m n : (m + 1) n], read by
the kernels through the index (wab_policy_grad_ppo_gather): no row is copied.  Everything is HIP
launches on one stream; the one host read per epoch (the printed loss, clip fraction and KL) is
optional: --quiet leaves it out.

    python examples/train_ppo.py [--envs 4096] [--steps 64] [--updates 20] [--epochs 4]
                                 [--minibatches 4] [--clip 0.2] [--value-clip 0.2] [--shuffle] [--packed]
                                 [--quiet]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # train_actor_critic.py's Policy

from wab_gym_amd.env import BatchedWolvesAndBushesEnv  # noqa: E402
from wab_gym_amd.policy import DeviceAdam, DevicePolicy  # noqa: E402
from wab_gym_amd.wrappers import PragmaticObsWrapper  # noqa: E402

from train_actor_critic import Policy  # noqa: E402,F401


def update(wrapper, policy, model, opt, T, epochs=4, minibatches=4, clip=0.2, value_clip=0.2, entropy_coef=0.0,
           report=None, shuffle=False, perm=None, packed=False):
    """One rollout segment and epochs x minibatches clipped steps (opt: a DeviceAdam, whose step()
    re-packs the policy's weights).  Minibatch m is the steps [m T / M, (m + 1) T / M) of the
    segment, a view; with shuffle, the rows perm[m n : (m + 1) n] of a permutation of the segment's
    T B rows drawn afresh each epoch into `perm` (an int32 [T B] device buffer, made here when not
    given), n = T B / M.  Returns the ppo_loss_and_grad results as a list of lists [epoch][minibatch]
    (device tensors: nothing here reads them); report(epoch, results) is called after each epoch.
    packed: the segment's feature rows are kept as 1 bit per feature (wab_rollout_policy_packed, 64
    bytes per row of the reference net instead of 1796) for the evaluate pass and every minibatch;
    the parameters after the update have the same bits."""
    if T % minibatches != 0:
        raise ValueError("the segment's %d steps do not split into %d minibatches" % (T, minibatches))
    r = wrapper.rollout_policy(policy, T, bootstrap_value=True, gae_lambda=0.95, whiten=True,
                               store_features="packed" if packed else True)
    feats = r["feature_bits"] if packed else r["features"]
    old_logp = policy.evaluate(feats, r["actions"])["logp"]
    step = T // minibatches
    rows_all = r["actions"].numel()
    n = rows_all // minibatches
    if shuffle and perm is None:
        perm = torch.empty(rows_all, dtype=torch.int32, device=feats.device)
    results = []
    for e in range(epochs):
        outs = []
        if shuffle:
            torch.randperm(rows_all, device=perm.device, dtype=torch.int32, out=perm)
        for m in range(minibatches):
            if shuffle:
                outs.append(policy.ppo_loss_and_grad(feats, r["actions"], r["advantage"], r["target"],
                                                     old_logp, clip=clip, old_value=r["value"],
                                                     value_clip=value_clip, into=model, reduction="mean",
                                                     entropy_coef=entropy_coef, rows=perm[m * n:(m + 1) * n]))
                opt.step()
                continue
            s = slice(m * step, (m + 1) * step)
            outs.append(policy.ppo_loss_and_grad(feats[s], r["actions"][s], r["advantage"][s], r["target"][s],
                                                 old_logp[s], clip=clip, old_value=r["value"][s],
                                                 value_clip=value_clip, into=model, reduction="mean",
                                                 entropy_coef=entropy_coef))
            opt.step()
        results.append(outs)
        if report is not None:
            report(e, outs)
    return results


def print_epoch(e, outs):
    """The optional host read: the epoch's mean loss, clip fraction and KL (synchronises)."""
    mean = [float(torch.stack([o[k] for o in outs]).mean()) for k in ("loss", "clip_fraction", "approx_kl")]
    print("  epoch %d: loss %.6f  clip fraction %.4f  approx kl %.3e" % (e, mean[0], mean[1], mean[2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--value-clip", type=float, default=0.2, help="0: no value clipping")
    ap.add_argument("--shuffle", action="store_true", help="minibatches from a fresh permutation of the rows per epoch")
    ap.add_argument("--packed", action="store_true", help="keep the segment's feature rows as 1 bit per feature")
    ap.add_argument("--quiet", action="store_true", help="no host read per epoch")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    env = BatchedWolvesAndBushesEnv(num_envs=args.envs, seed=0x5EED, device=dev)
    wrapper = PragmaticObsWrapper(env)
    wrapper.reset()
    torch.manual_seed(0)
    model = Policy(n_actions=env.n_actions).to(dev)
    policy = DevicePolicy(model, env)
    opt = DeviceAdam(policy, model, lr=3e-4, max_grad_norm=0.5)
    perm = torch.empty(args.steps * args.envs, dtype=torch.int32, device=dev) if args.shuffle else None
    for i in range(args.updates):
        if not args.quiet:
            print("update %d" % i)
        update(wrapper, policy, model, opt, args.steps, args.epochs, args.minibatches, args.clip, args.value_clip,
               report=None if args.quiet else print_epoch, shuffle=args.shuffle, perm=perm, packed=args.packed)
    policy.check()
    print("optimizer: %s" % (opt.stats(),))


if __name__ == "__main__":
    main()
