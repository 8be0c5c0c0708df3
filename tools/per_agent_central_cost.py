#!/usr/bin/env python3
"""Cost of per-agent actors beside the centralised critic (share_actor: false with critic_input: state) against the two
paths it joins, at 3v1, K = 5, D = 35, in alternating blocks of one process (tools/per_agent_cost.py's method), the shader clock probed before
and after.  `new` is PerAgentCentralCriticDevicePolicy / PerAgentCentralCriticDeviceLearner, `agents` the per-agent actors beside the critic on
the observation (PerAgentDevicePolicy / PerAgentDeviceLearner), `central` the shared actor beside the centralised critic
(CentralCriticDevicePolicy / CentralCriticDeviceLearner); `agents` is timed twice per round (agents, agents-again): the spread of one path
against itself in the same process, which a difference has to exceed.

  forward (actors + critic, sampled), value_only and act at 2 048 and 65 536 envs
  one collector step (env step + policy + the fused stores; a collect of 8 steps / 8) at 2 048 and 65 536 envs, predictor off
  one train_rollout at the reference default (2 048 envs x 64 steps, 4 epochs x 16 minibatches, predictor on)

    python tools/per_agent_central_cost.py [--blocks 5] [--calls 30] [--skip-large]
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/per_agent_central_cost.py --blocks 1 --calls 5 (a run of its own)."""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import hns_amd  # noqa: E402,F401
from hns_amd import abi, collector, config, learner  # noqa: E402
from hns_amd import policy as P  # noqa: E402

A, K, D = 3, 5, 35
BASE = "agents"


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


def report(what, times, per=1):
    med = {k: v[len(v) // 2] for k, v in times.items()}
    for k, v in times.items():
        print(f"  {what} {k:12s} median {med[k] / per * 1e3:10.1f} us  (min {v[0] / per * 1e3:.1f}, max {v[-1] / per * 1e3:.1f})  "
              f"x{med[k] / med[BASE]:.3f} of {BASE}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--skip-large", action="store_true", help="leave out the 65 536-env collector step")
    args = ap.parse_args()
    dev = torch.device("cuda")
    from hns_amd.env import HideAndSeek
    with open(abi.library_path(), "rb") as f:
        print(f"libhns.so sha256 {hashlib.sha256(f.read()).hexdigest()}")
    probe_env = HideAndSeek(config.make_cfg({"env": {"num_envs": 64}}), headless=True)

    def clock():
        probe = probe_env.clock_probe(2000)
        torch.cuda.synchronize()
        return probe_env.clock_mhz(probe)

    print(f"shader clock before: {clock():.0f} MHz")
    to = lambda d: {k: v.to(dev).contiguous() for k, v in d.items()}                         # noqa: E731

    def policies(dim):
        stacked, obs_critic = P.random_parameters_per_agent(dim, A, 0)
        shared, central = P.random_parameters_central(dim, A, 0)
        stacked, obs_critic, shared, central = to(stacked), to(obs_critic), to(shared), to(central)
        return {"new": P.PerAgentCentralCriticDevicePolicy(stacked, central), "agents": P.PerAgentDevicePolicy(stacked, obs_critic),
                "central": P.CentralCriticDevicePolicy(shared, central)}

    pol = policies(D)
    print("forward (actors + critic, sampled), value_only (the critic alone) and act (the actors alone):")
    for E in (2048, 65536):
        g = torch.Generator(device=dev).manual_seed(1)
        r = lambda *s: torch.randn(*s, device=dev, generator=g)                              # noqa: E731
        xs, xo, xc, sd = r(E, A, D), r(E, A, A - 1, 3), r(E, A, K, 5), r(E, A, D)

        def calls(**kw):
            fns = {"new": lambda: pol["new"].forward(xs, xo, xc, sd, **kw), "agents": lambda: pol["agents"].forward(xs, xo, xc, **kw),
                   "central": lambda: pol["central"].forward(xs, xo, xc, sd, **kw)}
            return {**fns, "agents-again": fns["agents"]}

        act = {k: (lambda p=p: p.act(xs, xo, xc)) for k, p in pol.items()}
        act["agents-again"] = act["agents"]
        with torch.no_grad():
            report(f"E={E:6d} forward   ", alternate(calls(), args.blocks, args.calls))
            report(f"E={E:6d} value_only", alternate(calls(value_only=True), args.blocks, args.calls))
            report(f"E={E:6d} act       ", alternate(act, args.blocks, args.calls))

    print(f"one collector step (a collect of 8 steps / 8; predictor off, so D = {abi.HNS_SELF_DIM}):")
    T = 8
    for E in (2048,) + (() if args.skip_large else (65536,)):
        envs, cols = [], {}
        for name, p in policies(abi.HNS_SELF_DIM).items():
            env = HideAndSeek(config.make_cfg({"num_agents": A, "env": {"num_envs": E}}, algo={"use_TP_net": 0, "critic_input": "state"}), headless=True)
            env.set_seed(3)
            envs.append(env)
            cols[name] = collector.DeviceCollector(env, p, T)
        fns = {k: c.collect for k, c in cols.items()}
        fns["agents-again"] = fns["agents"]
        report(f"E={E:6d} step      ", alternate(fns, args.blocks, max(2, args.calls // 8)), per=T)
        for env in envs:
            env.close()
        del cols, fns
        torch.cuda.empty_cache()

    print("one train_rollout at the reference default (2 048 envs x 64 steps, 4 epochs x 16 minibatches, predictor on):")
    import central_learner_cases as CC
    import learner_cases as LC
    import per_agent_cases as PA
    import per_agent_central_cases as PC
    big = {"ppo_epochs": 4, "num_minibatches": 16}
    st_o = LC.make_state(A, 3)
    ro = LC.to_device(LC.make_rollout(st_o, 2048, 64, A, 4), dev)
    tp = lambda: LC.clone_state(LC.make_state(A, 3), dev)["tp"]                              # noqa: E731
    g = torch.Generator(device=dev).manual_seed(5)
    ro_c = {**ro, "state_drones": torch.randn(2048, 64, A, D, device=dev, generator=g) * 0.7,
            "next_state_last": torch.randn(2048, A, D, device=dev, generator=g) * 0.7}
    st_n, st_c = PC.make_state(A, D, 3, dev, tp=tp()), CC.make_state(A, D, 3, dev, tp=tp())
    st_a = PA.clone_state(PA.make_state(A, 3), dev)
    Ln = learner.PerAgentCentralCriticDeviceLearner(st_n["actor"], st_n["critic"], {**PC.CFG, **big}, tp_net=st_n["tp"], value_normalizer=st_n["vn"])
    La = learner.PerAgentDeviceLearner(st_a["actor"], st_a["critic"], {**PA.CFG, **big}, tp_net=st_a["tp"], value_normalizer=st_a["vn"])
    Lc = learner.CentralCriticDeviceLearner(st_c["actor"], st_c["critic"], {**CC.CFG, **big}, tp_net=st_c["tp"], value_normalizer=st_c["vn"])
    fns = {"new": lambda: Ln.train_rollout(**ro_c), "agents": lambda: La.train_rollout(**ro), "central": lambda: Lc.train_rollout(**ro_c)}
    fns["agents-again"] = fns["agents"]
    report("train_rollout", alternate(fns, args.blocks, 2))
    print(f"shader clock after: {clock():.0f} MHz")
    probe_env.close()


if __name__ == "__main__":
    main()
