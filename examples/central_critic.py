#!/usr/bin/env python3
"""MAPPO with the centralised critic (algo.critic_input: state) on the device from end to end.

    python examples/central_critic.py --envs 64 --train-every 16 --iterations 3

env -> CentralCriticDevicePolicy -> DeviceCollector -> CentralCriticDeviceLearner.train_rollout (train_op on tensors) -> DeviceEvaluator,
the loop of examples/train_device.py with the critic that sees all agents in the obs critic's place.  The env is built with
`algo.critic_input: state`, so the step, reset and predictor kernels write ("agents", "state", "state_drones"); the collector hands it to
the policy and stores it beside the observation, and the learner's critic update and bootstrap value read it.  The critic is ONE encoder
row per env over the state — the A rows of state_drones through one embedding, then the cylinders — and v_out = Linear(128, A).  The
state's cylinders are agent 0's rows of the observation's (the reference's spec declares [K, 5], its env returns [A, K, 5]: DESIGN.md
§7.20).  The checkpoint is the reference's dict with the centralised critic's names; the script writes one, builds a second learner and
policy from it, and shows that both continue with the same bits."""
import argparse
import os
import sys
import tempfile

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hns_amd  # noqa: E402,F401
from hns_amd import collector, config, evaluator, learner, policy  # noqa: E402
from hns_amd.env import HideAndSeek  # noqa: E402

ALGO = {"use_TP_net": 1, "ppo_epochs": 4, "num_minibatches": 4, "TP_epochs": 1, "clip_param": 0.1, "entropy_coef": 0.001, "gamma": 0.995,
        "gae_lambda": 0.95, "max_grad_norm": 10.0, "normalize_advantages": True, "share_actor": True, "critic_input": "state",
        "actor": {"lr": 5e-4, "weight_decay": 0.0, "tanh": False}, "critic": {"lr": 5e-4, "weight_decay": 0.0, "use_huber_loss": True, "huber_delta": 10}}


def build(env, seed):
    """(actor, critic: name -> live Parameter under the reference's names; the policy; the learner) for `env`."""
    D = env.observation_spec[("agents", "observation", "state_self")].shape[-1]
    actor, critic = policy.random_parameters_central(D, env.num_agents, seed=seed)
    actor, critic = ({k: nn.Parameter(v.to(env.device)) for k, v in p.items()} for p in (actor, critic))
    net = policy.CentralCriticDevicePolicy(actor, critic, ALGO, seed=seed)
    learn = learner.CentralCriticDeviceLearner(actor, critic, ALGO, tp_net=env.TP, value_normalizer=learner.ValueNorm1().to(env.device),
                                               device_policy=net, generator=torch.Generator(device=env.device).manual_seed(seed))
    return critic, net, learn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--train-every", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    algo = {"use_TP_net": 1, "critic_input": "state"}            # the kernels write state_drones
    env = HideAndSeek(config.make_cfg({"env": {"num_envs": args.envs}}, algo=algo))
    env.set_seed(args.seed)
    critic, net, learn = build(env, args.seed)
    print(f"{env.num_agents} agents, one critic row per env: v_out.weight {tuple(critic['v_out.weight'].shape)}")
    collect = collector.DeviceCollector(env, net, args.train_every)
    state = torch.get_rng_state()
    eval_env = HideAndSeek(config.make_cfg({"env": {"num_envs": args.envs}}, algo=algo))
    torch.set_rng_state(state)
    evaluate = evaluator.DeviceEvaluator(eval_env, net, tp_net=env.TP).evaluate
    for i in range(args.iterations):
        st = collect.collect()
        info = learn.train_rollout(**st.learner_kwargs())        # train_op, on the storage's tensors (state_drones among them)
        print(f"iteration {i}: " + "  ".join(f"{k.split('/')[-1]} {v:+.4f}" for k, v in info.items()))
    stats = evaluate(seed=0)
    print("eval: " + "  ".join(f"{k} {stats[k]:.4f}" for k in ("eval/stats.success", "eval/stats.collision", "eval/stats.return")))

    # the reference's checkpoint dict: write it, train on; then resume a second learner and policy from the file and train the same rollout
    path = os.path.join(tempfile.mkdtemp(), "checkpoint_final.pt")
    torch.save(learn.state_dict(), path)
    drawn = learn.generator.get_state()
    ro = collect.collect().learner_kwargs()
    a = learn.train_rollout(**ro)
    critic2, net2, learn2 = build(env, args.seed + 1)            # other initial values: everything comes from the checkpoint
    learn2.load_state_dict(torch.load(path, map_location=env.device))
    learn2.generator.set_state(drawn)
    b = learn2.train_rollout(**ro)
    same = all(torch.equal(critic[k], critic2[k]) for k in critic) and a == b
    eval_pol = policy.CentralCriticDevicePolicy.from_checkpoint(learn2.state_dict(), ALGO, device=env.device)
    td = env.reset()
    same = same and torch.equal(eval_pol.value(td), net.value(td))
    print(f"resumed from {os.path.basename(path)}: the resumed learner's next update and critic are {'bit for bit' if same else 'NOT'} the original's")
    eval_env.close()
    env.close()
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
