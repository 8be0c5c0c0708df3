#!/usr/bin/env python3
"""MAPPO on the device from end to end: env -> DevicePolicy -> DeviceCollector -> DeviceLearner, the loop scripts/train.py runs with the
reference's SyncDataCollector and MAPPOPolicy.train_op (random initial networks of the reference's architecture).

    python examples/train_device.py --envs 2048 --train-every 64 --iterations 10"""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hns_amd  # noqa: E402,F401
from hns_amd import collector, config, learner, policy  # noqa: E402
from hns_amd.env import HideAndSeek  # noqa: E402

ALGO = {"use_TP_net": 1, "ppo_epochs": 4, "num_minibatches": 16, "TP_epochs": 1, "clip_param": 0.1, "entropy_coef": 0.001, "gamma": 0.995,
        "gae_lambda": 0.95, "max_grad_norm": 10.0, "normalize_advantages": True, "share_actor": True, "critic_input": "obs",
        "actor": {"lr": 5e-4, "weight_decay": 0.0, "tanh": False}, "critic": {"lr": 5e-4, "weight_decay": 0.0, "use_huber_loss": True, "huber_delta": 10}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--train-every", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    env = HideAndSeek(config.make_cfg({"env": {"num_envs": args.envs}}, algo={"use_TP_net": 1}))
    env.set_seed(args.seed)
    D = env.observation_spec[("agents", "observation", "state_self")].shape[-1]
    # name -> live Parameter under the reference's names: the learner updates them in place, the policy re-packs when they move
    actor, critic = ({k: nn.Parameter(v.to(env.device)) for k, v in p.items()} for p in policy.random_parameters(D, env.num_agents, seed=args.seed))
    net = policy.DevicePolicy(actor, critic, ALGO, seed=args.seed)
    learn = learner.DeviceLearner(actor, critic, ALGO, tp_net=env.TP, value_normalizer=learner.ValueNorm1().to(env.device), device_policy=net)
    collect = collector.DeviceCollector(env, net, args.train_every)
    for i in range(args.iterations):
        info = learn.train_rollout(**collect.collect().learner_kwargs())
        stats, episodes = collect.episode_stats()
        print(f"iteration {i}: " + "  ".join(f"{k.split('/')[-1]} {v:+.4f}" for k, v in info.items()))
        if episodes:
            print(f"    {episodes} episodes: return {stats['return']:+.3f}  success {stats['success']:.3f}  collision {stats['collision']:.3f}")
    env.close()


if __name__ == "__main__":
    main()
