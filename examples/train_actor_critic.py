"""actor_critic.py's training loop with every step on the device: the closed-loop rollout
(wab_rollout_policy), the GAE advantages and value targets (wab_gae), the loss and its parameter
gradients (wab_policy_grad) and, with --device-adam, the optimizer step and the re-pack of the
policy's weights (wab_policy_adam_step); without it the optimizer is torch's.

    python examples/train_actor_critic.py [--envs 4096] [--steps 64] [--updates 20] [--device-adam]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wab_gym_amd.env import BatchedWolvesAndBushesEnv  # noqa: E402
from wab_gym_amd.policy import DeviceAdam, DevicePolicy  # noqa: E402
from wab_gym_amd.wrappers import PragmaticObsWrapper  # noqa: E402


class Policy(torch.nn.Module):
    """actor_critic.Policy's five Linears (the device policy runs its forward)."""

    def __init__(self, in_features=449, n_actions=5):
        super().__init__()
        self.affine1 = torch.nn.Linear(in_features, 128)
        self.affine2 = torch.nn.Linear(128, 150)
        self.affine3 = torch.nn.Linear(150, 128)
        self.action_head = torch.nn.Linear(128, n_actions)
        self.value_head = torch.nn.Linear(128, 1)


def update(wrapper, policy, model, opt, T, entropy_coef=0.0):
    """One rollout segment and one optimizer step; returns loss_and_grad's result."""
    r = wrapper.rollout_policy(policy, T, bootstrap_value=True, gae_lambda=0.95, whiten=True)
    out = policy.loss_and_grad(r["features"], r["actions"], r["advantage"], r["target"], into=model,
                               reduction="mean", entropy_coef=entropy_coef)
    opt.step()
    policy.load(model)
    return out


def update_device(wrapper, policy, model, opt, T, entropy_coef=0.0):
    """The same with opt a DeviceAdam: its step() also re-packs the policy's weights, so the whole
    update is HIP launches on one stream."""
    r = wrapper.rollout_policy(policy, T, bootstrap_value=True, gae_lambda=0.95, whiten=True)
    out = policy.loss_and_grad(r["features"], r["actions"], r["advantage"], r["target"], into=model,
                               reduction="mean", entropy_coef=entropy_coef)
    opt.step()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--device-adam", action="store_true",
                    help="step with DeviceAdam (clip at 0.5) instead of torch's Adam")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    env = BatchedWolvesAndBushesEnv(num_envs=args.envs, seed=0x5EED, device=dev)
    wrapper = PragmaticObsWrapper(env)
    wrapper.reset()
    torch.manual_seed(0)
    model = Policy(n_actions=env.n_actions).to(dev)
    policy = DevicePolicy(model, env)
    if args.device_adam:
        opt, step = DeviceAdam(policy, model, lr=3e-4, max_grad_norm=0.5), update_device
    else:
        opt, step = torch.optim.Adam(model.parameters(), lr=3e-4), update
    for i in range(args.updates):
        out = step(wrapper, policy, model, opt, args.steps)
        print("update %d: loss %.6f  policy %.4f  value %.4f  entropy %.4f"
              % (i, float(out["loss"]), float(out["loss_policy"]), float(out["loss_value"]), float(out["entropy"])))
    policy.check()
    if args.device_adam:
        print("optimizer: %s" % (opt.stats(),))


if __name__ == "__main__":
    main()
