#!/usr/bin/env python3
"""Cost of recurrent per-agent actors (share_actor: False with actor.rnn / critic.rnn; hns_amd.policy.PerAgentRecurrentDevicePolicy; DESIGN.md
§7.17) against what it replaces, at 3v1, K = 5, D = 35, in alternating blocks of ONE process (tools/per_agent_cost.py's method), the shader
clock probed before and after:

  forward (both networks, sampled) and act_step (the actor, the mode) at 2 048 and 65 536 envs, the states in place:
      per-agent   PerAgentRecurrentDevicePolicy: hns_policy_forward_rnn_agents / hns_policy_act_rnn_agents
      slices      A RecurrentDevicePolicy calls, one per agent's slice, each on the whole observation and state — the only device route
                  before (a shared policy cannot take one agent's [E, 1, ...] rows: the state_others key belongs to the layout)
      shared      ONE RecurrentDevicePolicy call on the same shapes (the floor: the same tiles and FLOPs, one pair of images instead of A + 1,
                  contiguous state rows)
  one collector step (DeviceCollector.collect() over 16 steps, rnn_seq_len 16, the predictor on) and one 800-step DeviceEvaluator.evaluate()
      with the per-agent recurrent policy against the shared recurrent policy, at 2 048 and 65 536 envs

    python tools/per_agent_rnn_cost.py [--blocks 5] [--calls 30] [--only-device] [--skip-loops]
    python tools/per_agent_rnn_cost.py --existing LABEL     # the paths that existed before, one line (alternating processes, two trees)
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/per_agent_rnn_cost.py --only-device --blocks 1 --calls 5 (a run of its own)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import hns_amd  # noqa: E402,F401
from hns_amd import collector, config, evaluator  # noqa: E402
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


def report(what, times, base, unit=1e3, name="us"):
    med = {k: v[len(v) // 2] for k, v in times.items()}
    for k, v in times.items():
        print(f"  {what} {k:10s} median {med[k] * unit:10.1f} {name}  (min {v[0] * unit:.1f}, max {v[-1] * unit:.1f})  x{med[k] / med[base]:.3f} of {base}")


def shared_recurrent(seed=0):
    actor, critic = P.random_parameters(D, A, seed)
    actor.update(P.random_rnn_parameters(seed + 1))
    critic.update(P.random_rnn_parameters(seed + 2))
    return actor, critic


def stacked_recurrent(seed=0):
    actors, critic = P.random_parameters_per_agent(D, A, seed)
    actors.update(P.random_rnn_parameters_per_agent(A, seed + 1))
    critic.update(P.random_rnn_parameters(seed + 2))
    return actors, critic


def obs_and_states(E, dev, n_states):
    g = torch.Generator(device=dev).manual_seed(1)
    xs, xo, xc = torch.randn(E, A, D, device=dev, generator=g), torch.randn(E, A, A - 1, 3, device=dev, generator=g), torch.randn(E, A, K, 5, device=dev, generator=g)
    return xs, xo, xc, [torch.zeros(E, A, 128, device=dev) for _ in range(n_states)]


def existing(label, blocks, calls):
    """The paths that existed before this configuration: RecurrentDevicePolicy.forward and PerAgentDevicePolicy.forward at 65 536 envs,
    medians of `blocks` blocks; run from a tree's own copy of this file, so each process measures its own tree's Python and library."""
    dev = torch.device("cuda")
    E = 65536
    xs, xo, xc, h = obs_and_states(E, dev, 2)
    actor, critic = shared_recurrent()
    rec = P.RecurrentDevicePolicy({k: v.to(dev) for k, v in actor.items()}, {k: v.to(dev) for k, v in critic.items()})
    actors, crit = P.random_parameters_per_agent(D, A, 0)
    per = P.PerAgentDevicePolicy({k: v.to(dev) for k, v in actors.items()}, {k: v.to(dev) for k, v in crit.items()})
    t = alternate({"rnn": lambda: rec.forward(xs, xo, xc, actor_state=h[0], critic_state=h[1], out_states=(h[0], h[1])),
                   "agents": lambda: per.forward(xs, xo, xc)}, blocks, calls)
    print(f"{label} forward_rnn_us {t['rnn'][len(t['rnn']) // 2] * 1e3:.1f} forward_agents_us {t['agents'][len(t['agents']) // 2] * 1e3:.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--only-device", action="store_true", help="the per-agent and the shared entries alone, no loops (profiler runs)")
    ap.add_argument("--skip-loops", action="store_true", help="leave out the collector and the evaluator")
    ap.add_argument("--existing", metavar="LABEL", help="RecurrentDevicePolicy.forward and PerAgentDevicePolicy.forward alone, one line")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("per_agent_rnn_cost: no GPU — nothing is measured without one")
    if args.existing:
        return existing(args.existing, args.blocks, args.calls)
    dev = torch.device("cuda")
    from hns_amd.env import HideAndSeek
    probe_env = HideAndSeek(config.make_cfg({"env": {"num_envs": 64}}), headless=True)

    def clock():
        probe = probe_env.clock_probe(2000)
        torch.cuda.synchronize()
        return probe_env.clock_mhz(probe)

    print(f"shader clock before: {clock():.0f} MHz")
    actors, critic = stacked_recurrent()
    actors, critic = {k: v.to(dev) for k, v in actors.items()}, {k: v.to(dev) for k, v in critic.items()}
    per = P.PerAgentRecurrentDevicePolicy(actors, critic)
    slices = [P.RecurrentDevicePolicy({k: v[a] for k, v in actors.items()}, critic) for a in range(A)]
    shared = slices[0]
    print("forward (actor + critic, sampled) and act_step (actor, mode), the states in place:")
    for E in (2048, 65536):
        xs, xo, xc, h = obs_and_states(E, dev, 6 + 2 * A)
        out = torch.empty(E, A, 4, device=dev)
        fwd = {"per-agent": lambda: per.forward(xs, xo, xc, actor_state=h[0], critic_state=h[1], out_states=(h[0], h[1])),
               "shared": lambda: shared.forward(xs, xo, xc, actor_state=h[2], critic_state=h[3], out_states=(h[2], h[3]))}
        act = {"per-agent": lambda: per.act_step(xs, xo, xc, state=h[4], out=out, out_state=h[4]),
               "shared": lambda: shared.act_step(xs, xo, xc, state=h[5], out=out, out_state=h[5])}
        if not args.only_device:
            # the user keeps agent a's rows of call a: every call carries its own pair of states
            fwd["slices"] = lambda: [pol.forward(xs, xo, xc, actor_state=h[6 + a], critic_state=h[3], out_states=(h[6 + a], h[3])) for a, pol in enumerate(slices)]
            act["slices"] = lambda: [pol.act_step(xs, xo, xc, state=h[6 + A + a], out=out, out_state=h[6 + A + a]) for a, pol in enumerate(slices)]
        with torch.no_grad():
            report(f"E={E:6d} forward ", alternate(fwd, args.blocks, args.calls), "shared")
            report(f"E={E:6d} act_step", alternate(act, args.blocks, args.calls), "shared")
        del xs, xo, xc, h, out, fwd, act
        torch.cuda.empty_cache()

    if not (args.only_device or args.skip_loops):
        print("one collector step (collect() over 16 steps / 16, rnn_seq_len 16) and one 800-step evaluate(), the predictor on:")
        for E in (2048, 65536):
            cfg = {"num_agents": A, "cylinder": {"obs_max_cylinder": K}, "env": {"num_envs": E, "max_episode_length": 800}}
            envs = []
            for _ in range(2):
                torch.manual_seed(1)                             # the predictor's initial weights come from the global generator
                envs.append(HideAndSeek(config.make_cfg(cfg, algo={"use_TP_net": 1}), headless=True))
            Dtp = envs[0].observation_spec[("agents", "observation", "state_self")].shape[-1]
            sa, sc = P.random_parameters(Dtp, A, 2)
            sa.update(P.random_rnn_parameters(3))
            sc.update(P.random_rnn_parameters(4))
            pa, pc = P.random_parameters_per_agent(Dtp, A, 2)
            pa.update(P.random_rnn_parameters_per_agent(A, 3))
            pc.update(P.random_rnn_parameters(4))
            edev = envs[0].device
            pols = {"per-agent": P.PerAgentRecurrentDevicePolicy(pa, pc, device=edev, seed=4), "shared": P.RecurrentDevicePolicy(sa, sc, device=edev, seed=4)}
            cols = {k: collector.DeviceCollector(env, pols[k], 16, rnn_seq_len=16) for k, env in zip(pols, envs)}
            t = alternate({k: c.collect for k, c in cols.items()}, args.blocks, 4)
            report(f"E={E:6d} collector step (D {Dtp})", {k: [x / 16 for x in v] for k, v in t.items()}, "shared")
            evs = {k: evaluator.DeviceEvaluator(env, pols[k]) for k, env in zip(pols, envs)}
            t = alternate({k: (lambda e=e: e.evaluate(seed=5)) for k, e in evs.items()}, min(args.blocks, 3), 1)
            report(f"E={E:6d} evaluate(), 800 steps  ", t, "shared", unit=1.0, name="ms")
            for env in envs:
                env.close()
            del envs, cols, evs, pols
            torch.cuda.empty_cache()
    print(f"shader clock after: {clock():.0f} MHz")
    probe_env.close()


if __name__ == "__main__":
    main()
