#!/usr/bin/env python3
"""Heterogeneous recurrent pursuers: MAPPO with share_actor: False AND actor.rnn / critic.rnn — one actor and one actor GRU per agent, the critic
and its GRU shared — collected and evaluated on the device.

    python examples/per_agent_recurrent.py --envs 64 --steps 16 --seq-len 8
    python examples/per_agent_recurrent.py --checkpoint checkpoint_final.pt     # the reference's dict (MAPPOPolicy.state_dict())

env -> PerAgentRecurrentDevicePolicy -> DeviceCollector(rnn_seq_len=) -> DeviceEvaluator: the loop of examples/recurrent_policy.py with the
stacked actor in the shared one's place.  This is the configuration the reference's recurrent update is written for (its vmap over dim 0 of
`actor_params`), so a checkpoint it trains with an rnn holds stacked recurrent actors: `actor_params` with every leaf [A, ...], the `rnn.*`
leaves among them.  The collector carries both rnn states [N, A, 128] on the device and stores `is_init` per step and the states going into
every segment; the evaluator carries ONE actor state in place.  The collector and the evaluator are the ones every policy uses.

Training this configuration on the device is not built yet (every learner refuses the policy: DESIGN-open-items.md #13); the stored rollout is
what a torch update over hns_amd.encoder / hns_amd.rnn per agent would read.  The script saves the checkpoint dict, loads it into a second
policy and shows that both act with the same bits."""
import argparse
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hns_amd  # noqa: E402,F401
from hns_amd import collector, config, evaluator, policy  # noqa: E402
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
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    task = {"env": {"num_envs": args.envs, "max_episode_length": args.episode}}
    env = HideAndSeek(config.make_cfg(task, algo={"use_TP_net": 1}))
    env.set_seed(args.seed)
    if args.checkpoint:
        ckpt = torch.load(args.checkpoint, map_location=env.device, weights_only=False)
        net = policy.PerAgentRecurrentDevicePolicy.from_checkpoint(ckpt, ALGO, device=env.device, seed=args.seed)
    else:
        ckpt, net = build(env, args.seed)
    print(f"{net.num_agents} recurrent actors, stacked: rnn.cell.weight_hh {tuple(net.actor_rnn['weight_hh'].shape)}, scale {tuple(net.scale.shape)}; "
          f"the critic's {tuple(net.critic_rnn['weight_hh'].shape)}")

    collect = collector.DeviceCollector(env, net, args.steps, rnn_seq_len=args.seq_len)
    storage = collect.collect()
    rk = storage.recurrent_kwargs()
    print(f"collected [{args.envs} envs x {args.steps} steps]: is_init {tuple(rk['is_init'].shape)} ({int(rk['is_init'].sum())} set), the states going "
          f"into {args.steps // args.seq_len} segments {tuple(rk['actor_rnn_state'].shape)}, reward mean {float(storage.data['reward'].mean()):+.4f}")

    state = torch.get_rng_state()
    eval_env = HideAndSeek(config.make_cfg(task, algo={"use_TP_net": 1}))
    torch.set_rng_state(state)
    stats = evaluator.DeviceEvaluator(eval_env, net, tp_net=env.TP).evaluate(seed=0)
    print("eval: " + "  ".join(f"{k} {stats[k]:.4f}" for k in ("eval/stats.success", "eval/stats.collision", "eval/stats.return")))

    # the reference's checkpoint dict: save it, load it into a second policy, and both act with the same bits from the same state
    path = os.path.join(tempfile.mkdtemp(), "checkpoint_final.pt")
    torch.save({k: {n: v.detach().cpu() for n, v in ckpt[k].items()} for k in ("actor_params", "critic")}, path)
    again = policy.PerAgentRecurrentDevicePolicy.from_checkpoint(path, ALGO, device=env.device, seed=args.seed)
    obs = env.reset()[("agents", "observation")]
    x = (obs["state_self"], obs["state_others"], obs["cylinders"])
    h = 0.5 * torch.randn(args.envs, net.num_agents, 128, device=env.device)
    (a0, s0), (a1, s1) = net.act_step(*x, state=h), again.act_step(*x, state=h)
    same = torch.equal(a0, a1) and torch.equal(s0, s1)
    differ = all(not torch.equal(a0[:, 0], a0[:, a]) for a in range(1, net.num_agents))
    print(f"loaded from {os.path.basename(path)}: the second policy's actions and states are {'bit for bit' if same else 'NOT'} the first's; "
          f"the agents' actions {'differ' if differ else 'do NOT differ'} (each pursuer acts from its own slice)")
    eval_env.close()
    env.close()
    if not (same and differ):
        sys.exit(1)


if __name__ == "__main__":
    main()
