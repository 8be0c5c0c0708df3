#!/usr/bin/env python3
"""Heterogeneous recurrent pursuers: MAPPO with share_actor: False AND actor.rnn / critic.rnn — one actor and one actor GRU per agent, the critic
and its GRU shared — collected, evaluated and trained on the device.

    python examples/per_agent_recurrent.py --envs 64 --steps 16 --seq-len 8
    python examples/per_agent_recurrent.py --envs 64 --steps 16 --seq-len 8 --learner --updates 2     # ... and trained
    python examples/per_agent_recurrent.py --checkpoint checkpoint_final.pt     # the reference's dict (MAPPOPolicy.state_dict())

env -> PerAgentRecurrentDevicePolicy -> DeviceCollector(rnn_seq_len=) -> DeviceEvaluator: the loop of examples/recurrent_policy.py with the
stacked actor in the shared one's place.  This is the configuration the reference's recurrent update is written for (its vmap over dim 0 of
`actor_params`), so a checkpoint it trains with an rnn holds stacked recurrent actors: `actor_params` with every leaf [A, ...], the `rnn.*`
leaves among them.  The collector carries both rnn states [N, A, 128] on the device and stores `is_init` per step and the states going into
every segment; the evaluator carries ONE actor state in place.  The collector and the evaluator are the ones every policy uses.

--learner: train through `learner.PerAgentRecurrentDeviceLearner` — one `train_rollout` per rollout: the bootstrap value, the
targets, the env's trajectory predictor, `--updates` PPO epochs of 4 minibatches of segments through rnn_train.update_actor_rnn_per_agent (the
encoder op, the GRU op and the head entry on the stacked tensors, ONE ClippedAdam step over the 29 stacked tensors) and update_critic_rnn.
Before the first step it recomputes the first minibatch's log-probabilities from the stored states and flags and prints max |ratio - 1|,
which is 0 up to rounding.  Under a launcher (WORLD_SIZE set) --learner makes the script one rank of a data-parallel run:
--envs is the WHOLE job's env count, each rank steps its `sharding.env_shard` slice and `learner.DataParallelPerAgentRecurrentLearner(group="world")`
performs one update on the union of the ranks' minibatches of segments; rank 0 prints.  The script saves the checkpoint dict, loads it into a second policy and shows that both act with the same bits."""
import argparse
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hns_amd  # noqa: E402,F401
from hns_amd import collector, config, evaluator, learner, policy, rnn_train, sharding  # noqa: E402
from hns_amd.env import HideAndSeek  # noqa: E402

ALGO = {"use_TP_net": 1, "share_actor": False, "critic_input": "obs", "actor": {"tanh": False, "rnn": {"cls": "gru", "train_seq_len": 8}},
        "critic": {"rnn": {"cls": "gru", "train_seq_len": 8}}}


def build(env, seed):
    """(the checkpoint dict's two entries under the reference's names, the policy) for `env`: A independently initialised recurrent actors."""
    D = env.observation_spec[("agents", "observation", "state_self")].shape[-1]
    actors, critic = policy.random_parameters_per_agent(D, env.num_agents, seed=seed)
    actors.update(policy.random_rnn_parameters_per_agent(env.num_agents, seed + 1))
    critic.update(policy.random_rnn_parameters(seed + 2))
    actors["act_dist.fc_mean.weight"] = actors["act_dist.fc_mean.weight"] * 30.0          # actions of order 0.3: the drones move
    actors, critic = ({k: v.to(env.device) for k, v in p.items()} for p in (actors, critic))
    return {"actor_params": actors, "critic": critic}, policy.PerAgentRecurrentDevicePolicy(actors, critic, ALGO, seed=seed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--seq-len", type=int, default=8)
    ap.add_argument("--episode", type=int, default=40, help="max_episode_length of the two envs")
    ap.add_argument("--checkpoint", default=None, help="a MAPPOPolicy.state_dict() file with stacked recurrent actor_params")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--learner", action="store_true", help="train through PerAgentRecurrentDeviceLearner: one train_rollout per rollout, two rollouts")
    ap.add_argument("--updates", type=int, default=2, help="PPO epochs per rollout (--learner)")
    args = ap.parse_args()
    rank, world = 0, 1
    if args.learner and "WORLD_SIZE" in os.environ:              # one rank of a data-parallel run
        import torch.distributed as dist
        rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
        dist.init_process_group(os.environ.get("HNS_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    offset, envs = sharding.env_shard(args.envs, world, rank)
    say = print if rank == 0 else (lambda *a, **k: None)
    torch.manual_seed(args.seed)
    task = {"env": {"num_envs": envs, "max_episode_length": args.episode}}
    env = HideAndSeek(config.make_cfg(task, algo={"use_TP_net": 1}), env_index_offset=offset)
    env.set_seed(args.seed)
    if args.checkpoint:
        ckpt = torch.load(args.checkpoint, map_location=env.device, weights_only=False)
        net = policy.PerAgentRecurrentDevicePolicy.from_checkpoint(ckpt, ALGO, device=env.device, seed=args.seed)
    else:
        ckpt, net = build(env, args.seed)
    say(f"{net.num_agents} recurrent actors, stacked: rnn.cell.weight_hh {tuple(net.actor_rnn['weight_hh'].shape)}, scale {tuple(net.scale.shape)}; "
          f"the critic's {tuple(net.critic_rnn['weight_hh'].shape)}")

    collect = collector.DeviceCollector(env, net, args.steps, rnn_seq_len=args.seq_len)
    storage = collect.collect()
    rk = storage.recurrent_kwargs()
    say(f"collected [{envs} envs x {args.steps} steps]: is_init {tuple(rk['is_init'].shape)} ({int(rk['is_init'].sum())} set), the states going "
          f"into {args.steps // args.seq_len} segments {tuple(rk['actor_rnn_state'].shape)}, reward mean {float(storage.data['reward'].mean()):+.4f}")

    if args.learner:
        algo = {**ALGO, "ppo_epochs": args.updates, "num_minibatches": 4, "actor": {**ALGO["actor"], "rnn": {"cls": "gru", "train_seq_len": args.seq_len}},
                "critic": {"rnn": {"cls": "gru", "train_seq_len": args.seq_len}}}
        if "WORLD_SIZE" in os.environ:                           # every rank permutes its own segments from its own generator
            make, more = learner.DataParallelPerAgentRecurrentLearner, {"group": "world", "generator": torch.Generator(device=env.device).manual_seed(rank)}
        else:
            make, more = learner.PerAgentRecurrentDeviceLearner, {}
        lrn = make(ckpt["actor_params"], ckpt["critic"], algo, tp_net=env.TP, value_normalizer=learner.ValueNorm1().to(env.device), device_policy=net,
                   **more)
        for it in range(2):
            kw = storage.learner_kwargs()
            if it == 0:                                          # the first minibatch before any step: the stored log-probabilities, recomputed
                segs = torch.arange(max(1, envs * (args.steps // args.seq_len) // 4), device=env.device)
                res = rnn_train.policy_loss_and_grad_rnn_per_agent(ckpt["actor_params"], kw["obs_self"], kw["obs_others"], kw["obs_cylinders"],
                                                                   rk["actor_rnn_state"], rk["is_init"], kw["action"], kw["log_probs"], kw["reward"],
                                                                   segment=segs, seq_len=args.seq_len)
                old = kw["log_probs"].reshape(-1, args.seq_len, net.num_agents, 1)[segs]
                say(f"first minibatch, before any step: max |ratio - 1| = {float((torch.exp(res.log_probs - old) - 1).abs().max()):.3e}")
            info = lrn.train_rollout(**kw, **rk)
            say(f"rollout {it}: " + "  ".join(f"{k.split('/')[-1]} {v:+.5f}" for k, v in info.items()))
            storage = collect.collect()
            rk = storage.recurrent_kwargs()

    state = torch.get_rng_state()
    eval_env = HideAndSeek(config.make_cfg(task, algo={"use_TP_net": 1}), env_index_offset=offset)
    torch.set_rng_state(state)
    stats = evaluator.DeviceEvaluator(eval_env, net, tp_net=env.TP).evaluate(seed=0)
    say("eval: " + "  ".join(f"{k} {stats[k]:.4f}" for k in ("eval/stats.success", "eval/stats.collision", "eval/stats.return")))

    # the reference's checkpoint dict: save it, load it into a second policy, and both act with the same bits from the same state
    path = os.path.join(tempfile.mkdtemp(), "checkpoint_final.pt")
    torch.save({k: {n: v.detach().cpu() for n, v in ckpt[k].items()} for k in ("actor_params", "critic")}, path)
    again = policy.PerAgentRecurrentDevicePolicy.from_checkpoint(path, ALGO, device=env.device, seed=args.seed)
    obs = env.reset()[("agents", "observation")]
    x = (obs["state_self"], obs["state_others"], obs["cylinders"])
    h = 0.5 * torch.randn(envs, net.num_agents, 128, device=env.device)
    (a0, s0), (a1, s1) = net.act_step(*x, state=h), again.act_step(*x, state=h)
    same = torch.equal(a0, a1) and torch.equal(s0, s1)
    differ = all(not torch.equal(a0[:, 0], a0[:, a]) for a in range(1, net.num_agents))
    say(f"loaded from {os.path.basename(path)}: the second policy's actions and states are {'bit for bit' if same else 'NOT'} the first's; "
          f"the agents' actions {'differ' if differ else 'do NOT differ'} (each pursuer acts from its own slice)")
    eval_env.close()
    env.close()
    if world > 1 or (args.learner and "WORLD_SIZE" in os.environ):
        torch.distributed.destroy_process_group()
    if not (same and differ):
        sys.exit(1)


if __name__ == "__main__":
    main()
