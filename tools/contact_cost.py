#!/usr/bin/env python3
"""Cost of the contact response (task.contact_response, include/hns.h): contact off against on inside ONE process, alternating timed blocks
(tools/ab_env.py switches environment variables and cannot switch a task option).  Each block times `steps` back-to-back hns_step launches of
one env with hipEvents around the block (GPU time per step, launch gaps included; the batch sizes here keep the queue full).
  contact_cost.py [--steps=2000 --blocks=7]
prints one line per shape and setting: median / min / max per-step time over the blocks, and the on / off ratio of the medians."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import hns_amd  # noqa: E402,F401
from hns_amd import config  # noqa: E402
from hns_amd.env import HideAndSeek  # noqa: E402

SHAPES = [(65536, 3, 8), (2048, 3, 5), (65536, 6, 16)]     # (envs, pursuers, cylinder slots)
steps, blocks = 2000, 7
for a in sys.argv[1:]:
    if a.startswith("--steps="):
        steps = int(a.split("=")[1])
    if a.startswith("--blocks="):
        blocks = int(a.split("=")[1])

for E, A, CYL in SHAPES:
    envs = []
    for on in (0, 1):
        cfg = config.make_cfg({"num_agents": A, "cylinder": {"max_num": CYL, "min_num": CYL}, "env": {"num_envs": E, "max_episode_length": 1000000},
                               "contact_response": on})
        e = HideAndSeek(cfg)
        e.set_seed(3)
        e.reset()
        envs.append(e)
    act = torch.randn(E, A, 4, device=envs[0].device) * 0.5
    t = [[] for _ in envs]
    for b in range(blocks + 1):
        for i, e in enumerate(envs):
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s0.record()
            for _ in range(steps):
                assert e._lib.hns_step(e._env, act.data_ptr(), e._stream()) == 0
            s1.record()
            torch.cuda.synchronize()
            if b:                                                   # block 0 warms up
                t[i].append(s0.elapsed_time(s1) / steps * 1e3)
    med = [float(np.median(x)) for x in t]
    for on, ti, e in zip((0, 1), t, envs):
        print(f"E={E} A={A} C={CYL}  contact_response={on}  mapping={e.step_mapping:5s}  median {np.median(ti):7.2f} us per step  "
              f"(min {min(ti):.2f}, max {max(ti):.2f}; {blocks} blocks of {steps})")
    assert all(e.check_finite() for e in envs)
    print(f"E={E} A={A} C={CYL}  on / off = {med[1] / med[0]:.3f}")
    del envs
    torch.cuda.empty_cache()
