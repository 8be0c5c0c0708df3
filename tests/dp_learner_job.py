#!/usr/bin/env python3
"""One rank of test_hip_dp_learner.py::test_two_ranks_on_one_gpu_over_gloo, started by torch.distributed.run: the HIP env on this rank's env
slice, DevicePolicy, DeviceCollector and DeviceLearner(group="world") with the predictor on — 4 envs x 8 steps a rank, one epoch of one
minibatch.  Every rank writes rank<r>.pt under --out (the start the group's rank 0 broadcast, its own rollout, its parameters after the
update); rank 0 prints ONE JSON line with every rank's sha256 over its parameters and its info row.  Ranks share cuda:<LOCAL_RANK modulo the
devices present>; the backend is HNS_DIST_BACKEND (gloo on one card: a correctness run, not a performance number)."""
import argparse
import hashlib
import json
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import hns_amd  # noqa: E402,F401
import learner_cases as LC  # noqa: E402
from hns_amd import collector, config, learner, policy, sharding  # noqa: E402
from hns_amd.env import HideAndSeek  # noqa: E402

ENVS, STEPS, A = 4, 8, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
    dist.init_process_group(os.environ.get("HNS_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    offset, count = sharding.env_shard(ENVS * world, world, rank)
    torch.manual_seed(100 + rank)                                # the predictor's initial weights: rank 0's reach every rank at construction
    env = HideAndSeek(config.make_cfg({"num_agents": A, "env": {"num_envs": count}}, algo={"use_TP_net": 1}), headless=True, env_index_offset=offset)
    env.set_seed(3)
    cfg = dict(LC.CFG, ppo_epochs=1, num_minibatches=1)
    state = LC.make_state(A, 81 + rank, "cuda")                  # other weights on every rank, until the broadcast
    pol = policy.DevicePolicy(state["actor"], state["critic"], cfg, seed=4 + rank)
    L = learner.DeviceLearner(state["actor"], state["critic"], cfg, tp_net=env.TP, value_normalizer=learner.ValueNorm1().to("cuda"),
                              generator=torch.Generator(device="cuda").manual_seed(5 + rank), device_policy=pol, group="world")
    cpu = lambda t: t.detach().cpu().clone() if torch.is_tensor(t) else (tuple(cpu(x) for x in t) if isinstance(t, tuple) else t)   # noqa: E731
    start = {"actor": {k: cpu(v) for k, v in state["actor"].items()}, "critic": {k: cpu(v) for k, v in state["critic"].state_dict().items()},
             "tp": {k: cpu(v) for k, v in env.TP.state_dict().items()},
             "tp_args": [env.tp_frame_dim, 3 * env.tp_future_step, env.tp_future_step, int(env.TP.window_step)]}
    kw = collector.DeviceCollector(env, pol, STEPS).collect().learner_kwargs()
    rollout = {k: cpu(v) for k, v in kw.items()}
    info = L.train_rollout(**kw)
    torch.cuda.synchronize()
    final = {k: cpu(v) for k, v in LC.state_tensors(dict(state, tp=env.TP, vn=L.value_normalizer), {}).items()}
    digest = hashlib.sha256(b"".join(final[k].numpy().tobytes() for k in sorted(final))).hexdigest()
    torch.save({"start": start, "cfg": cfg, "rollout": rollout, "final": final}, os.path.join(args.out, f"rank{rank}.pt"))
    box = [None] * world
    dist.all_gather_object(box, (digest, info))
    if rank == 0:
        print(json.dumps({"digests": [d for d, _ in box], "infos": [i for _, i in box]}))
    env.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
