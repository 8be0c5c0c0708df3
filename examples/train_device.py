#!/usr/bin/env python3
"""MAPPO on the device from end to end: env -> DevicePolicy -> DeviceCollector -> DeviceLearner, the loop scripts/train.py runs with the
reference's SyncDataCollector and MAPPOPolicy.train_op (random initial networks of the reference's architecture).

    python examples/train_device.py --envs 2048 --train-every 64 --iterations 10 --eval-interval 5 --save-interval 5 --checkpoint-dir runs/a

Evaluation (scripts/train.py:207-264, :283-285, :310-312) runs every --eval-interval iterations and once after the loop, on a SEPARATE env of
--eval-envs envs that takes the training env's predictor (hns_amd.evaluator), so training is exactly what it is without it.  Checkpoints
(:288-292, :315-318) are the learner's state_dict: checkpoint_<frames>.pt every --save-interval iterations and checkpoint_final.pt at the
end; --resume loads one before the loop.

Under a launcher (WORLD_SIZE set) the script is one rank of a data-parallel run:

    python -m torch.distributed.run --nproc-per-node 8 examples/train_device.py --envs 16384

--envs is then the WHOLE job's env count: each rank steps its `sharding.env_shard` slice, the learner's ranks perform one update on the union
of their minibatches (DeviceLearner(group="world")), and rank 0 alone prints, evaluates and writes checkpoints.  The backend is
HNS_DIST_BACKEND (default nccl, RCCL on ROCm; gloo runs several ranks on one card as a correctness run)."""
import argparse
import os
import sys

import torch
import torch.distributed as dist
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hns_amd  # noqa: E402,F401
from hns_amd import collector, config, evaluator, learner, policy, sharding  # noqa: E402
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
    ap.add_argument("--eval-interval", type=int, default=0, help="evaluate every this many iterations and once at the end (0: never)")
    ap.add_argument("--eval-envs", type=int, default=None, help="envs of the evaluation env (default: --envs)")
    ap.add_argument("--eval-seed", type=int, default=0)
    ap.add_argument("--save-interval", type=int, default=0, help="write checkpoint_<frames>.pt every this many iterations (0: never)")
    ap.add_argument("--checkpoint-dir", default=None, help="where checkpoints go (checkpoint_final.pt is written whenever this is set)")
    ap.add_argument("--resume", default=None, metavar="PATH", help="a checkpoint to load before the loop")
    args = ap.parse_args()
    rank, world = 0, int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" in os.environ:
        rank = int(os.environ["RANK"])
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
        dist.init_process_group(os.environ.get("HNS_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    first = rank == 0
    offset, envs = sharding.env_shard(args.envs, world, rank)
    torch.manual_seed(args.seed)
    env = HideAndSeek(config.make_cfg({"env": {"num_envs": envs}}, algo={"use_TP_net": 1}), env_index_offset=offset)
    env.set_seed(args.seed)
    D = env.observation_spec[("agents", "observation", "state_self")].shape[-1]
    # name -> live Parameter under the reference's names: the learner updates them in place, the policy re-packs when they move
    actor, critic = ({k: nn.Parameter(v.to(env.device)) for k, v in p.items()} for p in policy.random_parameters(D, env.num_agents, seed=args.seed))
    net = policy.DevicePolicy(actor, critic, ALGO, seed=args.seed + rank)                       # every rank samples its own noise
    learn = learner.DeviceLearner(actor, critic, ALGO, tp_net=env.TP, value_normalizer=learner.ValueNorm1().to(env.device), device_policy=net,
                                  generator=torch.Generator(device=env.device).manual_seed(args.seed + rank) if world > 1 else None,
                                  group="world" if "WORLD_SIZE" in os.environ else None)
    if args.resume:
        learn.load_state_dict(torch.load(args.resume, map_location=env.device))
    collect = collector.DeviceCollector(env, net, args.train_every)
    evaluate = None
    if args.eval_interval > 0 and first:
        state = torch.get_rng_state()                            # the evaluation env's predictor is initialised from torch's generator:
        eval_env = HideAndSeek(config.make_cfg({"env": {"num_envs": args.eval_envs or args.envs}}, algo={"use_TP_net": 1}))
        torch.set_rng_state(state)                               # ... training draws what it draws without an evaluation env
        evaluate = evaluator.DeviceEvaluator(eval_env, net, tp_net=env.TP).evaluate
    if args.checkpoint_dir and first:
        os.makedirs(args.checkpoint_dir, exist_ok=True)

    def report(frames):
        info = evaluate(seed=args.eval_seed)
        print(f"    eval at {frames} frames: " + "  ".join(f"{k} {info[k]:.4f}" for k in ("eval/stats.success", "eval/stats.collision", "eval/stats.return")))

    frames = 0
    for i in range(args.iterations):
        info = learn.train_rollout(**collect.collect().learner_kwargs())
        frames += args.envs * args.train_every
        stats, episodes = collect.episode_stats()
        if world > 1:                                            # one learner: every rank holds the same info row
            rows = [None] * world
            dist.all_gather_object(rows, info)
            assert all(r == rows[0] for r in rows), f"iteration {i}: the ranks' info rows differ: {rows}"
        if not first:                                            # (the episode statistics printed below are rank 0's envs')
            continue
        print(f"iteration {i}: " + "  ".join(f"{k.split('/')[-1]} {v:+.4f}" for k, v in info.items()))
        if episodes:
            print(f"    {episodes} episodes: return {stats['return']:+.3f}  success {stats['success']:.3f}  collision {stats['collision']:.3f}")
        if evaluate is not None and i % args.eval_interval == 0:
            report(frames)
        if args.checkpoint_dir and args.save_interval > 0 and i % args.save_interval == 0:
            torch.save(learn.state_dict(), os.path.join(args.checkpoint_dir, f"checkpoint_{frames}.pt"))
    if evaluate is not None:
        report(frames)
        eval_env.close()
    if args.checkpoint_dir and first:
        torch.save(learn.state_dict(), os.path.join(args.checkpoint_dir, "checkpoint_final.pt"))
    env.close()
    if "WORLD_SIZE" in os.environ:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
