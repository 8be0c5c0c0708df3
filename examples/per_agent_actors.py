#!/usr/bin/env python3
"""Heterogeneous pursuers: MAPPO with share_actor: False — one actor per agent, the critic shared — on the device from end to end.

    python examples/per_agent_actors.py --envs 64 --train-every 16 --iterations 3

env -> PerAgentDevicePolicy -> DeviceCollector -> PerAgentDeviceLearner.train_rollout (train_op on tensors) -> DeviceEvaluator, the loop of examples/train_device.py with
the stacked actor in the shared one's place: the actor's parameters are A independently initialised actors stacked over the agents (every
tensor [A, ...], as the reference's `actor_params` with share_actor: False), each pursuer acts from and trains its own slice, and ONE Adam
and one gradient clip run over the stacked tensors.  The collector and the evaluator are the ones every policy uses.  The checkpoint is the
reference's dict (MAPPOPolicy.state_dict(): "actor_params" the stacked tensors, "critic", "TP", "value_normalizer") plus the optimisers; the
script writes one, builds a second learner and policy from it, and shows that both continue with the same bits.

Under a launcher (WORLD_SIZE set, e.g. torchrun --nproc-per-node 2 examples/per_agent_actors.py) the script is one rank of a data-parallel run
(DESIGN.md §7.19): --envs is the WHOLE job's env count, each rank steps its `sharding.env_shard` slice, and
`learner.DataParallelPerAgentLearner(group="world")` performs one update on the union of the ranks' minibatches — every rank ends each
iteration with the same stacked actor.  Rank 0 prints."""
import argparse
import os
import sys
import tempfile

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hns_amd  # noqa: E402,F401
from hns_amd import collector, config, evaluator, learner, policy, sharding  # noqa: E402
from hns_amd.env import HideAndSeek  # noqa: E402

ALGO = {"use_TP_net": 1, "ppo_epochs": 4, "num_minibatches": 4, "TP_epochs": 1, "clip_param": 0.1, "entropy_coef": 0.001, "gamma": 0.995,
        "gae_lambda": 0.95, "max_grad_norm": 10.0, "normalize_advantages": True, "share_actor": False, "critic_input": "obs",
        "actor": {"lr": 5e-4, "weight_decay": 0.0, "tanh": False}, "critic": {"lr": 5e-4, "weight_decay": 0.0, "use_huber_loss": True, "huber_delta": 10}}


def build(env, seed, rank=0, group=None):
    """(stacked actor, critic: name -> live Parameter under the reference's names; the policy; the learner) for `env`.  group: this process is
    one rank of a data-parallel run — the learner is DataParallelPerAgentLearner, and every rank samples its own noise and permutations."""
    D = env.observation_spec[("agents", "observation", "state_self")].shape[-1]
    actors, critic = policy.random_parameters_per_agent(D, env.num_agents, seed=seed)
    actors, critic = ({k: nn.Parameter(v.to(env.device)) for k, v in p.items()} for p in (actors, critic))
    net = policy.PerAgentDevicePolicy(actors, critic, ALGO, seed=seed + rank)
    args = dict(tp_net=env.TP, value_normalizer=learner.ValueNorm1().to(env.device), device_policy=net,
                generator=torch.Generator(device=env.device).manual_seed(seed + rank))
    learn = learner.PerAgentDeviceLearner(actors, critic, ALGO, **args) if group is None else \
        learner.DataParallelPerAgentLearner(actors, critic, ALGO, group=group, **args)
    return actors, net, learn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--train-every", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    rank, world, group = 0, 1, None
    if "WORLD_SIZE" in os.environ:                               # one rank of a data-parallel run
        import torch.distributed as dist
        rank, world, group = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), "world"
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
        dist.init_process_group(os.environ.get("HNS_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    offset, envs = sharding.env_shard(args.envs, world, rank)
    say = print if rank == 0 else (lambda *a, **k: None)
    torch.manual_seed(args.seed)
    env = HideAndSeek(config.make_cfg({"env": {"num_envs": envs}}, algo={"use_TP_net": 1}), env_index_offset=offset)
    env.set_seed(args.seed)
    actors, net, learn = build(env, args.seed, rank, group)
    say(f"{env.num_agents} actors, stacked: fc_mean.weight {tuple(actors['act_dist.fc_mean.weight'].shape)}, scale {tuple(net.scale.shape)}")
    collect = collector.DeviceCollector(env, net, args.train_every)
    state = torch.get_rng_state()
    eval_env = HideAndSeek(config.make_cfg({"env": {"num_envs": envs}}, algo={"use_TP_net": 1}), env_index_offset=offset)
    torch.set_rng_state(state)
    evaluate = evaluator.DeviceEvaluator(eval_env, net, tp_net=env.TP).evaluate
    for i in range(args.iterations):
        info = learn.train_rollout(**collect.collect().learner_kwargs())    # train_op, on the storage's tensors
        say(f"iteration {i}: " + "  ".join(f"{k.split('/')[-1]} {v:+.4f}" for k, v in info.items()))
    stats = evaluate(seed=0)
    say("eval: " + "  ".join(f"{k} {stats[k]:.4f}" for k in ("eval/stats.success", "eval/stats.collision", "eval/stats.return")))
    spread = (actors["act_dist.log_std"].detach().max(0).values - actors["act_dist.log_std"].detach().min(0).values).max()
    say(f"the agents' log_std differ by up to {float(spread):.2e} after training (they started equal: each actor follows its own rows)")

    # the reference's checkpoint dict: write it, train on; then resume a second learner and policy from the file and train the same rollout
    path = os.path.join(tempfile.mkdtemp(), "checkpoint_final.pt")
    torch.save(learn.state_dict(), path)
    drawn = learn.generator.get_state()
    ro = collect.collect().learner_kwargs()
    a = learn.train_rollout(**ro)
    actors2, net2, learn2 = build(env, args.seed + 1, rank, group)    # other initial values: everything comes from the checkpoint
    learn2.load_state_dict(torch.load(path, map_location=env.device))  # (the predictor is the env's, shared: it goes back to the checkpoint too)
    learn2.generator.set_state(drawn)
    b = learn2.train_rollout(**ro)
    same = all(torch.equal(actors[k], actors2[k]) for k in actors) and a == b
    eval_pol = policy.PerAgentDevicePolicy.from_checkpoint(learn2.state_dict(), ALGO, device=env.device)
    obs = env.reset()[("agents", "observation")]
    same = same and torch.equal(eval_pol.act(obs["state_self"], obs["state_others"], obs["cylinders"]),
                                net.act(obs["state_self"], obs["state_others"], obs["cylinders"]))
    say(f"resumed from {os.path.basename(path)}: the resumed learner's next update and policy are {'bit for bit' if same else 'NOT'} the original's")
    eval_env.close()
    env.close()
    if group is not None:
        torch.distributed.destroy_process_group()
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
