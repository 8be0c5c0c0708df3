#!/usr/bin/env python3
"""Cost of the data-parallel learner path on ONE card: DeviceLearner.train_rollout with group=None against the same call with
a one-rank process group, which runs everything the data-parallel path adds — the gradient buckets, the critic's call split at the branch
decision (hns_critic_train_sums, hns_critic_train_grad_global), hns_actor_train_grad_global, two hns_grad_norm calls and three collectives per
minibatch pair — with nobody to wait for.  ONE process, alternating timed blocks (as tools/collector_cost.py): each block is `reps` rollouts
between two synchronisations, wall time per rollout.  Both arms start every block from the same weights and the same generator seed.

  dp_learner_cost.py [--envs 2048 --steps 64 --epochs 4 --minibatches 16 --blocks 5 --reps 2 --backend gloo]
  dp_learner_cost.py --per-agent    the same two arms with one actor per agent (share_actor: False): PerAgentDeviceLearner
                                    against DataParallelPerAgentLearner over the one-rank group (hns_actor_train_grad_agents_global, the
                                    bucket over the 23 stacked tensors)
  dp_learner_cost.py --profile      one plain update pair and hns_grad_norm at the actor's and the critic's bucket sizes, for a
                                    `rocprofv3 --kernel-trace --stats` run of its own: hns_grad_norm's two kernels beside the
                                    hns_critic_norm_kernel launch they replace

What this is not: a one-rank group measures the path's own cost, not a collective's — gloo moves host copies (a synchronisation per collective
that RCCL does not have), so its figure is an upper bound for the host side and says nothing about xGMI.  Two ranks over gloo on one card
(tests/test_hip_dp_learner.py) is a correctness run, not a performance number.  Weak scaling is DESIGN-open-items.md item 1."""
import argparse
import copy
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import hns_amd  # noqa: E402,F401
import learner_cost as LCOST  # noqa: E402  (the reference-default state and rollout of tools/learner_cost.py)
from hns_amd import actor_train as AT  # noqa: E402
from hns_amd import critic_train as CT  # noqa: E402
from hns_amd import learner  # noqa: E402
from hns_amd import policy_train as PT  # noqa: E402

CFG = {"use_TP_net": 1, "ppo_epochs": 4, "num_minibatches": 16, "TP_epochs": 1, "clip_param": 0.1, "entropy_coef": 0.001, "gamma": 0.995,
       "gae_lambda": 0.95, "max_grad_norm": 10.0, "normalize_advantages": True, "share_actor": True, "critic_input": "obs",
       "actor": {"lr": 5e-4, "weight_decay": 0.0, "tanh": False}, "critic": {"lr": 5e-4, "weight_decay": 0.0, "use_huber_loss": True, "huber_delta": 10}}


def make_learner(start, cfg, group, per_agent=False):
    """per_agent: the shared actor stacked over the agents (slice a shifted by 0.01 a: the agents differ), share_actor: False."""
    stack = (lambda v: torch.stack([v.detach() + 0.01 * a for a in range(LCOST.A)]).contiguous()) if per_agent else (lambda v: v.detach().clone())
    state = {"actor": {k: torch.nn.Parameter(stack(v)) for k, v in start["actor"].items()},
             "critic": {k: torch.nn.Parameter(v.detach().clone()) for k, v in start["critic"].items()}, "tp": copy.deepcopy(start["tp"]),
             "vn": copy.deepcopy(start["vn"])}
    args = dict(tp_net=state["tp"], value_normalizer=state["vn"], generator=torch.Generator(device="cuda").manual_seed(5))
    if not per_agent:
        return learner.DeviceLearner(state["actor"], state["critic"], cfg, group=group, **args)
    cfg = dict(cfg, share_actor=False)
    if group is None:
        return learner.PerAgentDeviceLearner(state["actor"], state["critic"], cfg, **args)
    return learner.DataParallelPerAgentLearner(state["actor"], state["critic"], cfg, group=group, **args)


def profile(start, ro, cfg):
    """One plain update pair (its hns_critic_norm_kernel launches are the ones replaced) and ten hns_grad_norm calls per bucket."""
    L = make_learner(start, cfg, None)
    L.train_rollout(**ro)
    for params in (AT.actor_parameters(L.actor), CT.critic_parameters(L.critic)):
        bucket = PT.GradBucket(params)
        bucket.flat.normal_()
        for _ in range(10):
            bucket.norm()
        print(f"bucket of {bucket.flat.numel()} floats: norm {float(bucket.norm()):.6f}")
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--backend", default="gloo", help="the one-rank group's backend (gloo; nccl is RCCL)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--per-agent", action="store_true", help="one actor per agent: PerAgentDeviceLearner against DataParallelPerAgentLearner")
    args = ap.parse_args()
    cfg = dict(CFG, ppo_epochs=args.epochs, num_minibatches=args.minibatches)
    start = LCOST.make_state("cuda", cfg)
    ro = LCOST.make_rollout("cuda", args.envs, args.steps, start)
    if args.profile:
        return profile(start, ro, dict(cfg, ppo_epochs=1, num_minibatches=1))
    store = os.path.join(tempfile.mkdtemp(), "store")
    dist.init_process_group(args.backend, rank=0, world_size=1, store=dist.FileStore(store, 1))
    arms = {"none": None, "group": dist.group.WORLD}
    times = {k: [] for k in arms}
    for k, g in arms.items():                                    # warm-up: workspaces, buckets, the kernels' first launches
        make_learner(start, cfg, g, args.per_agent).train_rollout(**ro)
    torch.cuda.synchronize()
    for b in range(args.blocks):
        for k in (list(arms) if b % 2 == 0 else list(arms)[::-1]):
            L = make_learner(start, cfg, arms[k], args.per_agent)
            L.train_rollout(**ro)                                # (the learner's own first call allocates; not timed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                L.train_rollout(**ro)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / args.reps * 1e3)
    pairs = args.epochs * args.minibatches
    print(f"{'PerAgentDeviceLearner / DataParallelPerAgentLearner' if args.per_agent else 'DeviceLearner'}.train_rollout, {args.envs} envs x {args.steps} steps x {LCOST.A} agents, {args.epochs} epochs x {args.minibatches} minibatches, predictor on; "
          f"{args.blocks} alternating blocks of {args.reps} rollouts, ms per rollout")
    for k, v in times.items():
        print(f"  group={'None' if k == 'none' else 'one rank (' + args.backend + ')':<16} median {statistics.median(v):9.3f}  min {min(v):9.3f}  max {max(v):9.3f}")
    d = statistics.median(times["group"]) - statistics.median(times["none"])
    print(f"  difference {d:+.3f} ms per rollout, {d / pairs * 1e3:+.1f} us per minibatch pair ({pairs} pairs); "
          f"spread of group=None over the blocks {max(times['none']) - min(times['none']):.3f} ms")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
