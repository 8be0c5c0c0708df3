#!/usr/bin/env python3
"""Centralised training, decentralised execution: MAPPO with share_actor: False AND critic_input: state — one actor per pursuer on its own
observation under ONE critic over the joint state — on the device from end to end.

    python examples/per_agent_central.py --envs 64 --train-every 16 --iterations 3

env -> PerAgentCentralCriticDevicePolicy -> DeviceCollector -> PerAgentCentralCriticDeviceLearner.train_rollout (train_op on tensors) ->
DeviceEvaluator: the loop of examples/per_agent_actors.py with examples/central_critic.py's critic.  The actor's parameters are A
independently initialised actors stacked over the agents (every tensor [A, ...]); the critic is ONE encoder row per env over the state — the A
rows of state_drones through one embedding, then the cylinders — and v_out = Linear(128, A).  The env is built with
`algo.critic_input: state`, so its kernels write ("agents", "state", "state_drones"); the collector hands it to the policy and stores it, and
the learner's critic update and bootstrap value read it.  Evaluation runs the actors alone (`act`): the critic is a training-time device.  The
checkpoint is the reference's dict (stacked "actor_params", "critic" under the centralised critic's names, "TP", "value_normalizer") plus the
optimisers; the script writes one, builds a second learner and policy from it, and shows that both continue with the same bits.
DESIGN.md §7.21."""
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
        "gae_lambda": 0.95, "max_grad_norm": 10.0, "normalize_advantages": True, "share_actor": False, "critic_input": "state",
        "actor": {"lr": 5e-4, "weight_decay": 0.0, "tanh": False}, "critic": {"lr": 5e-4, "weight_decay": 0.0, "use_huber_loss": True, "huber_delta": 10}}


def build(env, seed):
    """(stacked actor, critic: name -> live Parameter under the reference's names; the policy; the learner) for `env`."""
    D = env.observation_spec[("agents", "observation", "state_self")].shape[-1]
    actors = policy.random_parameters_per_agent(D, env.num_agents, seed=seed)[0]
    critic = policy.random_parameters_central(D, env.num_agents, seed=seed)[1]
    actors, critic = ({k: nn.Parameter(v.to(env.device)) for k, v in p.items()} for p in (actors, critic))
    net = policy.PerAgentCentralCriticDevicePolicy(actors, critic, ALGO, seed=seed)
    learn = learner.PerAgentCentralCriticDeviceLearner(actors, critic, ALGO, tp_net=env.TP, value_normalizer=learner.ValueNorm1().to(env.device),
                                                       device_policy=net, generator=torch.Generator(device=env.device).manual_seed(seed))
    return actors, critic, net, learn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--train-every", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    algo = {"use_TP_net": 1, "critic_input": "state", "share_actor": False}       # the kernels write state_drones
    env = HideAndSeek(config.make_cfg({"env": {"num_envs": args.envs}}, algo=algo))
    env.set_seed(args.seed)
    actors, critic, net, learn = build(env, args.seed)
    print(f"{env.num_agents} actors, stacked: fc_mean.weight {tuple(actors['act_dist.fc_mean.weight'].shape)}, scale {tuple(net.scale.shape)}; "
          f"one critic row per env: v_out.weight {tuple(critic['v_out.weight'].shape)}")
    collect = collector.DeviceCollector(env, net, args.train_every)
    state = torch.get_rng_state()
    eval_env = HideAndSeek(config.make_cfg({"env": {"num_envs": args.envs}}, algo=algo))
    torch.set_rng_state(state)
    evaluate = evaluator.DeviceEvaluator(eval_env, net, tp_net=env.TP).evaluate
    for i in range(args.iterations):
        info = learn.train_rollout(**collect.collect().learner_kwargs())        # train_op, on the storage's tensors (state_drones among them)
        print(f"iteration {i}: " + "  ".join(f"{k.split('/')[-1]} {v:+.4f}" for k, v in info.items()))
    stats = evaluate(seed=0)
    print("eval: " + "  ".join(f"{k} {stats[k]:.4f}" for k in ("eval/stats.success", "eval/stats.collision", "eval/stats.return")))
    spread = (actors["act_dist.log_std"].detach().max(0).values - actors["act_dist.log_std"].detach().min(0).values).max()
    print(f"the agents' log_std differ by up to {float(spread):.2e} after training (they started equal: each actor follows its own rows)")

    # the reference's checkpoint dict: write it, train on; then resume a second learner and policy from the file and train the same rollout
    path = os.path.join(tempfile.mkdtemp(), "checkpoint_final.pt")
    torch.save(learn.state_dict(), path)
    drawn = learn.generator.get_state()
    ro = collect.collect().learner_kwargs()
    a = learn.train_rollout(**ro)
    actors2, critic2, net2, learn2 = build(env, args.seed + 1)   # other initial values: everything comes from the checkpoint
    learn2.load_state_dict(torch.load(path, map_location=env.device))  # (the predictor is the env's, shared: it goes back to the checkpoint too)
    learn2.generator.set_state(drawn)
    b = learn2.train_rollout(**ro)
    same = all(torch.equal(actors[k], actors2[k]) for k in actors) and all(torch.equal(critic[k], critic2[k]) for k in critic) and a == b
    eval_pol = policy.PerAgentCentralCriticDevicePolicy.from_checkpoint(learn2.state_dict(), ALGO, device=env.device)
    td = env.reset()
    obs = td[("agents", "observation")]
    same = same and torch.equal(eval_pol.value(td), net.value(td)) and torch.equal(
        eval_pol.act(obs["state_self"], obs["state_others"], obs["cylinders"]), net.act(obs["state_self"], obs["state_others"], obs["cylinders"]))
    print(f"resumed from {os.path.basename(path)}: the resumed learner's next update, actors and critic are {'bit for bit' if same else 'NOT'} the original's")
    eval_env.close()
    env.close()
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
