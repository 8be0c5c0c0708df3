#!/usr/bin/env python3
"""Cost of a rollout step with the collector (hns_amd.collector.DeviceCollector: two hns_rollout_store launches per step, `done` read back
once per episode) against the same loop driven by hand, which is what a user wrote before the collector existed: one torch `copy_` per stored
tensor and `done.any()` read back on every step.  ONE process, alternating timed blocks; each block is `collects` rollouts of `steps` steps
between two synchronisations, wall time per step (host and device: the loop is what the user waits for).
  collector_cost.py [--steps=64 --collects=4 --blocks=7]
  collector_cost.py --profile=ENVS      (three collects of the collector alone at one shape, for a `rocprofv3 --kernel-trace --stats` run:
                                         the store kernel's own time)
prints, per shape: median / min / max per-step time of both loops and their ratio; the store launches per step of both; and the stores on
their own — one step's two hns_rollout_store launches against the same tensors' copy_ calls, back to back between hipEvents."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import hns_amd  # noqa: E402,F401
from hns_amd import collector, config, policy  # noqa: E402
from hns_amd.env import HideAndSeek  # noqa: E402
from hns_amd.tensordict_shim import TensorDict  # noqa: E402

SHAPES = [2048, 65536]                                           # envs; 3 pursuers, predictor on (the reference's defaults)
steps, collects, blocks, profile = 64, 4, 7, 0
for a in sys.argv[1:]:
    if a.startswith("--profile="):
        profile = int(a.split("=")[1])
    if a.startswith("--steps="):
        steps = int(a.split("=")[1])
    if a.startswith("--collects="):
        collects = int(a.split("=")[1])
    if a.startswith("--blocks="):
        blocks = int(a.split("=")[1])


class HandLoop:
    """The loop a user writes without the collector.  tests/test_hip_collector.py has its own HandLoop, the reference the collector is compared
    with bit for bit: a change to the loop's order belongs in both."""

    def __init__(self, env, net, T):
        self.env, self.net, self.T, self.cur, self.buf, self.copies = env, net, T, None, {}, 0

    def _put(self, name, t, v):
        if name not in self.buf:
            self.buf[name] = torch.zeros(v.shape[0], self.T, *v.shape[1:], dtype=v.dtype, device=v.device)
        self.buf[name][:, t].copy_(v)
        self.copies += 1

    def collect(self):
        env = self.env
        cur = self.cur if self.cur is not None else env.reset()
        for t in range(self.T):
            obs = cur[("agents", "observation")]
            out = self.net.forward(obs["state_self"], obs["state_others"], obs["cylinders"])
            for name, v in (("obs_self", obs["state_self"]), ("obs_others", obs["state_others"]), ("obs_cylinders", obs["cylinders"]),
                            ("action", out.action), ("log_probs", out.log_prob), ("state_value", out.value)):
                self._put(name, t, v)
            nxt = env.step(env.rand_step_input(out.action))["next"]
            done = nxt["done"]
            for name, v in (("reward", nxt[("agents", "reward")]), ("done", done), *((k, nxt[("agents", "TP", k)]) for k in collector.TP_KEYS)):
                self._put(name, t, v)
            if t == self.T - 1:
                nobs = nxt[("agents", "observation")]
                self.last = tuple(nobs[k].clone() for k in ("state_self", "state_others", "cylinders"))
                self.copies += 3
            if bool(done.any()):
                cur = env.reset(TensorDict({"_reset": done.clone()}, env.batch_size))
            else:
                cur = nxt
        self.cur = cur


def events_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


if profile:
    SHAPES, blocks, collects = [profile], 0, 3

for E in SHAPES:
    loops = []
    for kind in ("collector", "hand")[:1 if profile else 2]:
        torch.manual_seed(1)
        env = HideAndSeek(config.make_cfg({"env": {"num_envs": E}}, algo={"use_TP_net": 1}))
        env.set_seed(3)
        D = env.observation_spec[("agents", "observation", "state_self")].shape[-1]
        net = policy.DevicePolicy(*policy.random_parameters(D, env.num_agents, seed=2), device=env.device, seed=4)
        loops.append(collector.DeviceCollector(env, net, steps) if kind == "collector" else HandLoop(env, net, steps))
    if profile:
        for _ in range(collects):
            loops[0].collect()
        torch.cuda.synchronize()
        loops[0].env.close()
        break
    col, hand = loops
    t = [[], []]
    for b in range(blocks + 1):
        for i, loop in enumerate(loops):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(collects):
                loop.collect()
            torch.cuda.synchronize()
            if b:                                                    # block 0 warms up
                t[i].append((time.perf_counter() - t0) / (collects * steps) * 1e6)
    n = (blocks + 1) * collects * steps
    for name, ti in zip(("collector", "hand loop"), t):
        print(f"E={E} T={steps}  {name:9s}  median {np.median(ti):8.2f} us per step  (min {min(ti):.2f}, max {max(ti):.2f}; {blocks} blocks of {collects} x {steps} steps)")
    print(f"E={E} T={steps}  collector / hand loop = {np.median(t[0]) / np.median(t[1]):.3f}")
    print(f"E={E} T={steps}  store launches per step: collector {col.storage.launches / n:.3f} (hns_rollout_store)  hand loop {hand.copies / n:.3f} (copy_)  "
          f"done read-backs: collector {col.done_reads}, hand loop {n}")
    # the stores on their own: this step's sources into slot 0, back to back
    st, cur = col.storage, col._cur
    obs = cur[("agents", "observation")]
    out = col.policy.forward(obs["state_self"], obs["state_others"], obs["cylinders"])
    pre = {"obs_self": obs["state_self"], "obs_others": obs["state_others"], "obs_cylinders": obs["cylinders"], "action": out.action,
           "log_probs": out.log_prob, "state_value": out.value}
    nxt = col.env.step(col.env.rand_step_input(out.action))["next"]
    post = {"reward": nxt[("agents", "reward")], "done": nxt["done"], **{k: nxt[("agents", "TP", k)] for k in collector.TP_KEYS}}
    nbytes = sum(v[0].numel() * v.element_size() for v in (*pre.values(), *post.values())) * E

    def fused():
        st.store(0, pre)
        st.store(0, post)

    def copies():
        for k, v in (*pre.items(), *post.items()):
            st.data[k][:, 0].copy_(v)

    reps = 500 if E <= 4096 else 100
    f_us, c_us = events_us(fused, reps), events_us(copies, reps)
    print(f"E={E}  one step's stores ({nbytes / 1e6:.2f} MB): 2 hns_rollout_store launches {f_us:7.2f} us  11 copy_ launches {c_us:7.2f} us  "
          f"(back to back between events, {reps} repetitions)")
    for loop in loops:
        loop.env.close()
    del loops, col, hand, st
    torch.cuda.empty_cache()
