#!/usr/bin/env python3
"""A critic the fused update refuses — weight decay and an lr schedule — written in torch over hns_amd.encoder, on the device end to end:

    python examples/custom_head.py --envs 256 --steps 16 --updates 8

The rollout comes from DeviceCollector; the critic is an AttentionEncoder (HIP forward and backward under autograd), a torch nn.Linear(128, 1)
and nn.HuberLoss, stepped by torch.optim.AdamW(weight_decay=...) under StepLR.  update_critic raises for both (critic.weight_decay,
critic.lr_scheduler); everything but the encoder is a few flops per row, so torch is the right place for it."""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hns_amd  # noqa: E402,F401
from hns_amd import collector, config, gae, policy  # noqa: E402
from hns_amd.encoder import AttentionEncoder  # noqa: E402
from hns_amd.env import HideAndSeek  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--updates", type=int, default=8)
    args = ap.parse_args()
    torch.manual_seed(0)
    env = HideAndSeek(config.make_cfg({"env": {"num_envs": args.envs}}, algo={"use_TP_net": 1}))
    env.set_seed(0)
    dev, A = env.device, env.num_agents
    D = env.observation_spec[("agents", "observation", "state_self")].shape[-1]
    actor, critic = ({k: nn.Parameter(v.to(dev)) for k, v in p.items()} for p in policy.random_parameters(D, A, seed=0))
    net = policy.DevicePolicy(actor, critic, seed=0)
    kw = collector.DeviceCollector(env, net, args.steps).collect().learner_kwargs()
    with torch.no_grad():
        next_value = net.forward(*kw["next_obs_last"], value_only=True).value
    _, returns, _ = gae.rollout_targets(kw["reward"], kw["done"].unsqueeze(-1), kw["state_value"], next_value, 0.995, 0.95)
    returns = returns.reshape(args.envs * args.steps, A, 1)

    encoder, head = AttentionEncoder(D, A).to(dev), nn.Linear(128, 1).to(dev)
    opt = torch.optim.AdamW([*encoder.parameters(), *head.parameters()], lr=5e-4, weight_decay=0.01)
    schedule = torch.optim.lr_scheduler.StepLR(opt, step_size=4, gamma=0.5)
    loss_fn = nn.HuberLoss(delta=10.0)
    for u in range(args.updates):
        index = torch.randperm(args.envs * args.steps, device=dev)[:args.envs * args.steps // 4]
        values = head(encoder(kw["obs_self"], kw["obs_others"], kw["obs_cylinders"], index, check_index=False))    # the rollout, read in place
        loss = loss_fn(values, returns[index])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        schedule.step()
        print(f"update {u}: value loss {loss.item():.5f}  lr {schedule.get_last_lr()[0]:.2e}")
    env.close()


if __name__ == "__main__":
    main()
