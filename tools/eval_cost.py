#!/usr/bin/env python3
"""Cost of evaluation on the device (hns_amd.evaluator), ONE process, alternating blocks, 3v1, 5 observed cylinders, D 35:
  (a) hns_policy_act (the actor alone) against hns_policy_forward with HNS_POLICY_DETERMINISTIC (actor and critic) on the same inputs,
      back to back between hipEvents;
  (b) DeviceEvaluator.evaluate() over an episode against the flow a user writes from the reference's evaluate() (scripts/train.py:207-254):
      policy.forward(deterministic=True) -> env.step, the statistics stacked per step, then argmax over the stacked `done`, take_along_dim and
      nanmean — wall time between two synchronisations and peak allocated bytes above what was allocated before the run.
  eval_cost.py [--blocks=7 --episode=800 --envs=2048,65536]
The hand flow is given every help that does not change what it computes: the env stays in training mode (views, no per-step clones of the
observation), the 24 statistics are cloned as ONE [24, N] copy per step, and the gather and the means stay on the device with one copy to
the host at the end."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import hns_amd  # noqa: E402,F401
from hns_amd import abi, config, evaluator, policy  # noqa: E402
from hns_amd.env import HideAndSeek  # noqa: E402

SHAPES, blocks, episode = [2048, 65536], 7, 800
for a in sys.argv[1:]:
    if a.startswith("--blocks="):
        blocks = int(a.split("=")[1])
    if a.startswith("--episode="):
        episode = int(a.split("=")[1])
    if a.startswith("--envs="):
        SHAPES = [int(x) for x in a.split("=")[1].split(",")]


def events_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def hand_flow(env, net, seed):
    """The reference's evaluate() by hand; returns {"eval/stats.<name>": float}."""
    env.set_seed(seed)
    env.clear_carried_state()                                    # as evaluate() does: both arms run the same episodes
    td = env.reset()
    stats, dones = [], []
    for _ in range(env.max_episode_length):
        obs = td[("agents", "observation")]
        action = net.forward(obs["state_self"], obs["state_others"], obs["cylinders"], deterministic=True).action
        td = env.step(env.rand_step_input(action))["next"]
        stats.append(env._bufs["stats"].clone())                 # [24, N]: the 24 statistics in one copy
        dones.append(td["done"].clone())
    done = torch.stack(dones, dim=1)                             # [N, L, 1]
    traj = torch.stack(stats, dim=2)                             # [24, N, L]
    first_done = torch.argmax(done.long(), dim=1)                # [N, 1]
    first = torch.take_along_dim(traj, first_done.reshape(1, -1, 1), dim=2).squeeze(2)
    means = torch.nanmean(first, dim=1).cpu().tolist()
    return {evaluator.KEY + k: v for k, v in zip(abi.STAT_NAMES, means)}


def timed(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated() - base, out


for E in SHAPES:
    cfg = {"cylinder": {"obs_max_cylinder": 5}, "env": {"num_envs": E, "max_episode_length": episode}}
    envs = []
    for _ in range(2):
        torch.manual_seed(1)                                     # the predictor's initial weights come from the global generator
        envs.append(HideAndSeek(config.make_cfg(cfg, algo={"use_TP_net": 1})))
    D = envs[0].observation_spec[("agents", "observation", "state_self")].shape[-1]
    K = envs[0].obs_max_cylinder
    net = policy.DevicePolicy(*policy.random_parameters(D, envs[0].num_agents, seed=2), device=envs[0].device, seed=4)

    # (a) the two kernels on one observation
    envs[0].set_seed(3)
    obs = envs[0].reset()[("agents", "observation")]
    xs, xo, xc = obs["state_self"], obs["state_others"], obs["cylinders"]
    out = torch.empty(E, envs[0].num_agents, 4, device=envs[0].device)
    arms = [lambda: net.act(xs, xo, xc, out=out), lambda: net.forward(xs, xo, xc, deterministic=True)]
    assert torch.equal(arms[0](), arms[1]().action)
    reps = 300 if E <= 4096 else 60
    t = [[], []]
    for b in range(blocks + 1):
        for i, fn in enumerate(arms):
            us = events_us(fn, reps)
            if b:                                                # block 0 warms up
                t[i].append(us)
    for name, ti in zip(("hns_policy_act", "hns_policy_forward, deterministic"), t):
        print(f"E={E} D={D} K={K}  {name:34s} median {np.median(ti):8.2f} us per call  (min {min(ti):.2f}, max {max(ti):.2f}; {blocks} blocks of {reps} calls)")
    print(f"E={E} D={D} K={K}  act / forward = {np.median(t[0]) / np.median(t[1]):.3f}")

    # (b) an evaluation run
    ev = evaluator.DeviceEvaluator(envs[0], net)
    arms = [lambda: ev.evaluate(seed=5), lambda: hand_flow(envs[1], net, 5)]
    t, peak, res = [[], []], [0, 0], [None, None]
    for b in range(min(blocks, 3) + 1):
        for i, fn in enumerate(arms):
            ms, pk, res[i] = timed(fn)
            if b:
                t[i].append(ms)
                peak[i] = max(peak[i], pk)
    worst = max(abs(res[0][k] - res[1][k]) / max(abs(res[1][k]), 1e-30) for k in res[1] if np.isfinite(res[1][k]))
    for name, ti, pk in zip(("evaluate()", "hand flow"), t, peak):
        print(f"E={E} L={episode}  {name:10s} median {np.median(ti):9.2f} ms per run  (min {min(ti):.2f}, max {max(ti):.2f}; {len(ti)} runs)  "
              f"peak allocated {pk / 1e6:10.2f} MB")
    print(f"E={E} L={episode}  evaluate() / hand flow = {np.median(t[0]) / np.median(t[1]):.3f} in time, {peak[0] / max(peak[1], 1):.5f} in peak bytes; "
          f"host read-backs per run: evaluate() {ev.done_reads // (min(blocks, 3) + 1)}, hand flow 1; "
          f"largest relative difference of the means (fp64 sums against torch.nanmean's fp32) {worst:.1e}")
    for env in envs:
        env.close()
    del envs, ev, net, arms, obs, xs, xo, xc, out
    torch.cuda.empty_cache()
