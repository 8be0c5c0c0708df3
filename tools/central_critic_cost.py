#!/usr/bin/env python3
"""Cost of the centralised critic (critic_input: state) against the critic on the observation it replaces, at 3v1, K = 5,
D = 35, in alternating blocks of one process (tools/per_agent_cost.py's method), the shader clock probed before and after:

  forward (actor + critic, sampled) and the value_only call at 2 048 and 65 536 envs: CentralCriticDevicePolicy against DevicePolicy;
      `obs` is timed twice per block (obs, obs-again): the spread of one path against itself in the same process
  one minibatch of update_critic_central against update_critic at the reference default (8 192 env-steps, 24 576 values) and at
      262 144 env-steps (786 432 values)
  one train_rollout at the reference default (2 048 envs x 64 steps, 4 epochs x 16 minibatches, predictor on): CentralCriticDeviceLearner
      against DeviceLearner

    python tools/central_critic_cost.py [--blocks 5] [--calls 30] [--skip-large]
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/central_critic_cost.py --blocks 1 --calls 5 (a run of its own)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import hns_amd  # noqa: E402,F401
from hns_amd import config  # noqa: E402
from hns_amd import critic_train as CT  # noqa: E402
from hns_amd import policy as P  # noqa: E402

A, K, D = 3, 5, 35


def alternate(fns, blocks, calls):
    """{name: sorted ms per call over the blocks}: every function warmed, then blocks of `calls` calls in turn, host clock around a synchronise."""
    times = {k: [] for k in fns}
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / calls * 1e3)
    return {k: sorted(v) for k, v in times.items()}


def report(what, times, base):
    med = {k: v[len(v) // 2] for k, v in times.items()}
    for k, v in times.items():
        print(f"  {what} {k:10s} median {med[k] * 1e3:10.1f} us  (min {v[0] * 1e3:.1f}, max {v[-1] * 1e3:.1f})  x{med[k] / med[base]:.3f} of {base}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--skip-large", action="store_true", help="leave out the 262 144-env-step minibatch (6 GB of workspace for the obs critic)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    from hns_amd.env import HideAndSeek
    probe_env = HideAndSeek(config.make_cfg({"env": {"num_envs": 64}}), headless=True)

    def clock():
        probe = probe_env.clock_probe(2000)
        torch.cuda.synchronize()
        return probe_env.clock_mhz(probe)

    print(f"shader clock before: {clock():.0f} MHz")
    to = lambda d: {k: v.to(dev) for k, v in d.items()}                                      # noqa: E731
    actor, central = P.random_parameters_central(D, A, 0)
    _, obs_critic = P.random_parameters(D, A, 0)
    actor, central, obs_critic = to(actor), to(central), to(obs_critic)
    new, old = P.CentralCriticDevicePolicy(actor, central), P.DevicePolicy(actor, obs_critic)
    print("forward (actor + critic, sampled) and value_only (the critic alone):")
    for E in (2048, 65536):
        g = torch.Generator(device=dev).manual_seed(1)
        r = lambda *s: torch.randn(*s, device=dev, generator=g)                              # noqa: E731
        xs, xo, xc, sd = r(E, A, D), r(E, A, A - 1, 3), r(E, A, K, 5), r(E, A, D)
        fwd = {"central": lambda: new.forward(xs, xo, xc, sd), "obs": lambda: old.forward(xs, xo, xc), "obs-again": lambda: old.forward(xs, xo, xc)}
        val = {"central": lambda: new.forward(xs, xo, xc, sd, value_only=True), "obs": lambda: old.forward(xs, xo, xc, value_only=True),
               "obs-again": lambda: old.forward(xs, xo, xc, value_only=True)}
        with torch.no_grad():
            report(f"E={E:6d} forward   ", alternate(fwd, args.blocks, args.calls), "obs")
            report(f"E={E:6d} value_only", alternate(val, args.blocks, args.calls), "obs")

    print("one minibatch of the critic's update (gradient call + clipped Adam):")
    for envs, steps, mb in ((2048, 64, 16),) + (() if args.skip_large else ((65536, 64, 16),)):
        S = envs * steps
        B = S // mb
        g = torch.Generator(device=dev).manual_seed(2)
        r = lambda *s: torch.randn(*s, device=dev, generator=g)                              # noqa: E731
        xs, xo, xc, sd = r(envs, steps, A, D) * 0.7, r(envs, steps, A, A - 1, 3) * 0.5, r(envs, steps, A, K, 5) * 0.5, r(envs, steps, A, D) * 0.7
        bv, ret = r(envs, steps, A, 1) * 0.3, r(envs, steps, A, 1)
        idx = torch.randperm(S, device=dev, generator=g)[:B]
        pc = {k: nn.Parameter(v.clone()) for k, v in central.items()}
        po = {k: nn.Parameter(v.clone()) for k, v in obs_critic.items()}
        oc, oo = CT.make_optimizer(pc), CT.make_optimizer(po)
        fns = {"central": lambda: CT.update_critic_central(pc, sd, xc, bv, ret, oc, index=idx),
               "obs": lambda: CT.update_critic(po, xs, xo, xc, bv, ret, oo, index=idx),
               "obs-again": lambda: CT.update_critic(po, xs, xo, xc, bv, ret, oo, index=idx)}
        report(f"{B:7d} env-steps", alternate(fns, args.blocks, max(2, args.calls // (6 if B > 100000 else 2))), "obs")
        del xs, xo, xc, sd, bv, ret, pc, po, oc, oo
        torch.cuda.empty_cache()

    print("one train_rollout at the reference default (2 048 envs x 64 steps, 4 epochs x 16 minibatches, predictor on):")
    import central_learner_cases as CC
    import learner_cases as LC
    from hns_amd import learner
    cfg_o = {**LC.CFG, "ppo_epochs": 4, "num_minibatches": 16}
    cfg_c = {**cfg_o, "critic_input": "state"}
    st_o = LC.make_state(A, 3)
    ro = LC.to_device(LC.make_rollout(st_o, 2048, 64, A, 4), dev)
    st_o = LC.clone_state(st_o, dev)
    st_c = CC.make_state(A, D, 3, dev, tp=LC.clone_state(LC.make_state(A, 3), dev)["tp"])
    g = torch.Generator(device=dev).manual_seed(5)
    ro_c = {**ro, "state_drones": torch.randn(2048, 64, A, D, device=dev, generator=g) * 0.7,
            "next_state_last": torch.randn(2048, A, D, device=dev, generator=g) * 0.7}
    Lo = learner.DeviceLearner(st_o["actor"], st_o["critic"], cfg_o, tp_net=st_o["tp"], value_normalizer=st_o["vn"])
    Lc = learner.CentralCriticDeviceLearner(st_c["actor"], st_c["critic"], cfg_c, tp_net=st_c["tp"], value_normalizer=st_c["vn"])
    report("train_rollout", alternate({"central": lambda: Lc.train_rollout(**ro_c), "obs": lambda: Lo.train_rollout(**ro),
                                       "obs-again": lambda: Lo.train_rollout(**ro)}, args.blocks, 2), "obs")
    print(f"shader clock after: {clock():.0f} MHz")
    probe_env.close()


if __name__ == "__main__":
    main()
