#!/usr/bin/env python3
"""One rank of test_hip_dp_per_agent.py::test_two_ranks_on_one_gpu_over_gloo, started as a process of its own (--rank, --world, --store: the
file store the ranks meet at; --which plain | rnn): the HIP env on this rank's env slice (3 and 5 envs: unequal shards), one actor per agent
(policy.random_parameters_per_agent; with rnn the stacked GRUs beside them), the per-agent policy, DeviceCollector and
DataParallelPerAgentLearner / DataParallelPerAgentRecurrentLearner(group="world") with the env's predictor — two rollouts of 8 steps, one
epoch of two minibatches each.  Every rank writes rank<r>.json under --out: the sha256 over its networks right after the construction
broadcast, the sha256 over its networks, Adam states and ValueNorm1 after the updates, and its info rows.  All ranks share cuda:0; the
backend is HNS_DIST_BACKEND (default gloo: a correctness run on one card, not a performance number)."""
import argparse
import hashlib
import json
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import hns_amd  # noqa: E402,F401
from hns_amd import collector, config, learner, policy, tp_train  # noqa: E402
from hns_amd.env import HideAndSeek  # noqa: E402

ENVS, STEPS, SEQ = (3, 5), 8, 4
CFG = {"ppo_epochs": 1, "num_minibatches": 2, "share_actor": False, "critic_input": "obs"}
RNN = {"actor": {"rnn": {"cls": "gru", "train_seq_len": SEQ}}, "critic": {"rnn": {"cls": "gru", "train_seq_len": SEQ}}}


def _digest(tensors):
    return hashlib.sha256(b"".join(t.detach().cpu().contiguous().numpy().tobytes() for t in tensors)).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", choices=("plain", "rnn"), required=True)
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--store", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    rank, world, rnn = args.rank, args.world, args.which == "rnn"
    torch.cuda.set_device(0)
    dist.init_process_group(os.environ.get("HNS_DIST_BACKEND", "gloo"), rank=rank, world_size=world, store=dist.FileStore(args.store, world))
    count, offset = ENVS[rank], sum(ENVS[:rank])
    torch.manual_seed(100 + rank)                                # other weights (the predictor's too) on every rank, until the broadcast
    env = HideAndSeek(config.make_cfg({"env": {"num_envs": count}}, algo={"use_TP_net": 1}), headless=True, env_index_offset=offset)
    env.set_seed(3)
    A = env.num_agents
    D = env.observation_spec[("agents", "observation", "state_self")].shape[-1]
    actors, critic = policy.random_parameters_per_agent(D, A, seed=10 * rank)
    if rnn:
        actors.update(policy.random_rnn_parameters_per_agent(A, 10 * rank + 1))
        critic.update(policy.random_rnn_parameters(10 * rank + 2))
    actors["act_dist.fc_mean.weight"] = actors["act_dist.fc_mean.weight"] * 30.0          # actions of order 0.3: the drones move
    live = (lambda v: v) if rnn else torch.nn.Parameter          # (as the two examples hold them)
    actors, critic = ({k: live(v.to(env.device).contiguous()) for k, v in p.items()} for p in (actors, critic))
    cfg = {**CFG, **RNN} if rnn else CFG
    pol = (policy.PerAgentRecurrentDevicePolicy if rnn else policy.PerAgentDevicePolicy)(actors, critic, cfg, seed=4 + rank)
    make = learner.DataParallelPerAgentRecurrentLearner if rnn else learner.DataParallelPerAgentLearner
    lrn = make(actors, critic, cfg, tp_net=env.TP, value_normalizer=learner.ValueNorm1().to(env.device),
               generator=torch.Generator(device=env.device).manual_seed(5 + rank), device_policy=pol, group="world")
    nets = [*actors.values(), *critic.values(), *tp_train.parameters(env.TP)]
    start = _digest(nets)
    col = collector.DeviceCollector(env, pol, STEPS, **({"rnn_seq_len": SEQ} if rnn else {}))
    infos = []
    for _ in range(2):
        st = col.collect()
        infos.append(lrn.train_rollout(**st.learner_kwargs(), **(st.recurrent_kwargs() if rnn else {})))
    torch.cuda.synchronize()
    state = list(nets)
    for opt in (lrn.actor_opt, lrn.critic_opt, lrn.tp_opt):
        for s in opt.state_dict()["state"].values():
            state += [s["step"], s["exp_avg"], s["exp_avg_sq"]]
    vn = lrn.value_normalizer
    state += [vn.running_mean, vn.running_mean_sq, vn.debiasing_term]
    with open(os.path.join(args.out, f"rank{rank}.json"), "w") as f:
        json.dump({"start": start, "digest": _digest(state), "infos": infos, "envs": count}, f)
    env.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
