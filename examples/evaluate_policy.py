"""How good is a policy?  The sampled policy against the greedy one, each in one closed-loop
rollout on the device (wab_rollout_policy under the policy's action rule, wab_policy_set_action_rule):
every env starts a fresh episode, the policy acts for T steps, and the episodes that finished are
averaged (EpisodeMonitor).  The greedy rule takes the first maximum of the probabilities in place
of the keyed draw, inside the same launch: no probs leave the device, no argmax is run on them.

    python examples/evaluate_policy.py [--checkpoint model.pt] [--envs 4096] [--steps 256]
                                       [--temperature 1.0]

--checkpoint: a state dict of train_actor_critic.Policy saved with torch.save (the five Linears by
the reference's names); without it a freshly initialised model is evaluated.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # train_actor_critic.py's Policy

from wab_gym_amd.env import BatchedWolvesAndBushesEnv  # noqa: E402
from wab_gym_amd.monitor import EpisodeMonitor  # noqa: E402
from wab_gym_amd.policy import DevicePolicy  # noqa: E402
from wab_gym_amd.wrappers import PragmaticObsWrapper  # noqa: E402


def evaluate(wrapper, policy, T, mode, temperature=1.0):
    """One EpisodeMonitor.rollout_policy of T steps from a reset of every env, under
    policy.acting(mode=mode, temperature=temperature); the policy's own rule is back afterwards.
    Returns {"mean_return", "mean_length", "episodes"} of the episodes that finished inside the T
    steps (the means are NaN when none did: raise T).  wrapper: a PragmaticObsWrapper over the env
    the policy was made for."""
    monitor = EpisodeMonitor(wrapper, video_callable=False)
    monitor.reset()
    with policy.acting(mode=mode, temperature=temperature):
        monitor.rollout_policy(policy, T, store_features=False)
    rewards, lengths = monitor.get_episode_rewards(), monitor.get_episode_lengths()  # (synchronises)
    n = len(rewards)
    return {"mean_return": sum(rewards) / n if n else float("nan"),
            "mean_length": sum(lengths) / n if n else float("nan"), "episodes": n}


def main():
    from train_actor_critic import Policy

    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None, help="a state dict of train_actor_critic.Policy (torch.save)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--temperature", type=float, default=1.0, help="of the sampled run (the greedy one does not "
                                                                   "depend on it)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    env = BatchedWolvesAndBushesEnv(num_envs=args.envs, seed=0x5EED, device=dev)
    wrapper = PragmaticObsWrapper(env)
    torch.manual_seed(0)
    model = Policy(n_actions=env.n_actions).to(dev)
    if args.checkpoint is not None:
        model.load_state_dict(torch.load(args.checkpoint, map_location=dev))
    policy = DevicePolicy(model, env)
    for mode, tau in (("sample", args.temperature), ("greedy", 1.0)):
        r = evaluate(wrapper, policy, args.steps, mode, tau)
        print("%-6s (temperature %g): mean return %.4f  mean length %.2f  over %d episodes"
              % (mode, tau, r["mean_return"], r["mean_length"], r["episodes"]))


if __name__ == "__main__":
    main()
