#!/usr/bin/env python3
"""Cost of evaluating a recurrent policy on the device (hns_amd.evaluator with a RecurrentDevicePolicy), ONE process,
alternating blocks, 3v1, 5 observed cylinders, D 35 (the predictor on):
  (a) RecurrentDevicePolicy.act_step (hns_policy_act_rnn: the actor's encoder, GRU step and head) against forward(deterministic=True)
      (hns_policy_forward_rnn: both networks) on the same inputs, the states in place, back to back between hipEvents;
  (b) DeviceEvaluator.evaluate() over an episode against the flow a user writes from the reference's evaluate() (scripts/train.py:207-254):
      forward(deterministic=True) -> env.step with both states carried, the statistics stacked per step, then argmax over the stacked `done`,
      take_along_dim and nanmean — wall time between two synchronisations and peak allocated bytes above what was allocated before the run.
  eval_rnn_cost.py [--blocks=7 --episode=800 --envs=2048,65536 --only=act_step|forward]
`--only=act_step` (or forward) runs that kernel's blocks alone: the run to put under `rocprofv3 --kernel-trace --stats -- python
tools/eval_rnn_cost.py --only=act_step` for the kernel's own time.  The hand flow is given every help that does not change what it computes:
the env stays in training mode (views, no per-step clones of the observation), the states are updated in place, the 24 statistics are cloned
as ONE [24, N] copy per step, and the gather and the means stay on the device with one copy to the host at the end."""
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

SHAPES, blocks, episode, only = [2048, 65536], 7, 800, None
for a in sys.argv[1:]:
    if a.startswith("--blocks="):
        blocks = int(a.split("=")[1])
    if a.startswith("--episode="):
        episode = int(a.split("=")[1])
    if a.startswith("--envs="):
        SHAPES = [int(x) for x in a.split("=")[1].split(",")]
    if a.startswith("--only="):
        only = a.split("=")[1]
if not torch.cuda.is_available():
    sys.exit("eval_rnn_cost: no GPU — nothing is measured without one")


def events_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def hand_flow(env, net, seed):
    """The reference's evaluate() by hand for a recurrent policy; returns {"eval/stats.<name>": float}."""
    env.set_seed(seed)
    env.clear_carried_state()                                    # as evaluate() does: both arms run the same episodes
    td = env.reset()
    stats, dones = [], []
    states = (None, None)
    for _ in range(env.max_episode_length):
        obs = td[("agents", "observation")]
        out = net.forward(obs["state_self"], obs["state_others"], obs["cylinders"], actor_state=states[0], critic_state=states[1],
                          deterministic=True, out_states=states)
        states = (out.actor_state, out.critic_state)
        td = env.step(env.rand_step_input(out.action))["next"]
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
    A = envs[0].num_agents
    actor, critic = policy.random_parameters(D, A, seed=2)
    actor.update(policy.random_rnn_parameters(seed=3))
    critic.update(policy.random_rnn_parameters(seed=4))
    net = policy.RecurrentDevicePolicy(actor, critic, device=envs[0].device, seed=4)

    # (a) the two kernels on one observation, each carrying its own state in place
    envs[0].set_seed(3)
    obs = envs[0].reset()[("agents", "observation")]
    xs, xo, xc = obs["state_self"], obs["state_others"], obs["cylinders"]
    out = torch.empty(E, A, 4, device=envs[0].device)
    h = [torch.zeros(E, A, 128, device=envs[0].device) for _ in range(3)]
    arms = [lambda: net.act_step(xs, xo, xc, state=h[0], out=out, out_state=h[0]),
            lambda: net.forward(xs, xo, xc, actor_state=h[1], critic_state=h[2], deterministic=True, out_states=(h[1], h[2]))]
    names = ("hns_policy_act_rnn", "hns_policy_forward_rnn, deterministic")
    for _ in range(3):                                           # the two chains feed themselves: the same bits at every step
        assert torch.equal(arms[0]()[0], arms[1]().action) and torch.equal(h[0], h[1])
    if only:
        arms, names = ([arms[0]], names[:1]) if only == "act_step" else ([arms[1]], names[1:])
    reps = 300 if E <= 4096 else 60
    t = [[] for _ in arms]
    for b in range(blocks + 1):
        for i, fn in enumerate(arms):
            us = events_us(fn, reps)
            if b:                                                # block 0 warms up
                t[i].append(us)
    for name, ti in zip(names, t):
        print(f"E={E} D={D} K={K}  {name:38s} median {np.median(ti):8.2f} us per call  (min {min(ti):.2f}, max {max(ti):.2f}; {blocks} blocks of {reps} calls)")
    if not only:
        print(f"E={E} D={D} K={K}  act_step / forward = {np.median(t[0]) / np.median(t[1]):.3f}")

        # (b) an evaluation run
        ev = evaluator.DeviceEvaluator(envs[0], net)
        arms = [lambda: ev.evaluate(seed=5), lambda: hand_flow(envs[1], net, 5)]
        runs = min(blocks, 3)
        t, peak, res = [[], []], [0, 0], [None, None]
        for b in range(runs + 1):
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
              f"host read-backs per run: evaluate() {ev.done_reads // (runs + 1)}, hand flow 1; "
              f"largest relative difference of the means (fp64 sums against torch.nanmean's fp32) {worst:.1e}")
        del ev
    for env in envs:
        env.close()
    del envs, net, arms, obs, xs, xo, xc, out, h
    torch.cuda.empty_cache()
