#!/usr/bin/env python3
"""Cost of one actor per agent (share_actor: False) against what it replaces, at 3v1, K = 5, D = 35, in alternating blocks of one
process (tools/policy_cost.py's and tools/actor_update_cost.py's method), the shader clock probed before and after:

  forward / act at 2 048 and 65 536 envs: PerAgentDevicePolicy against
      shared    DevicePolicy on the same build (the floor: the same tiles and FLOPs; the weights are fetched A times instead of once)
      slices    A DevicePolicy calls, one per agent's slice on that agent's rows (what a user could do before)
      torch     the reference's flow on the same GPU, the actor looped over the agents' slices (policy.torch_forward per slice)
  one minibatch of update_actor_per_agent at 24 576 and 786 432 rows against the shared update_actor and the torch flow (the per-agent CPU
      path's statements on device tensors, torch.optim.Adam over the stacked tensors)
  one train_rollout at the reference default (2 048 envs x 64 steps, 4 epochs x 16 minibatches) against DeviceLearner

    python tools/per_agent_cost.py [--blocks 5] [--calls 30] [--skip-large] [--only-device]
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/per_agent_cost.py --only-device --blocks 1 --calls 5 (a run of its own)."""
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
from hns_amd import actor_train as AT  # noqa: E402
from hns_amd import config  # noqa: E402
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
        print(f"  {what} {k:10s} median {med[k] * 1e3:10.1f} us  (min {v[0] * 1e3:.1f}, max {v[-1] * 1e3:.1f})  x{med[k] / med[base]:.3f} of {base}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--skip-large", action="store_true", help="leave out the 786 432-row minibatch (6 GB of workspace per path)")
    ap.add_argument("--only-device", action="store_true", help="the two device paths alone (profiler runs)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    from hns_amd.env import HideAndSeek
    probe_env = HideAndSeek(config.make_cfg({"env": {"num_envs": 64}}), headless=True)

    def clock():
        probe = probe_env.clock_probe(2000)
        torch.cuda.synchronize()
        return probe_env.clock_mhz(probe)

    print(f"shader clock before: {clock():.0f} MHz")

    actors, critic = P.random_parameters_per_agent(D, A, 0)
    actors, critic = {k: v.to(dev) for k, v in actors.items()}, {k: v.to(dev) for k, v in critic.items()}
    per = P.PerAgentDevicePolicy(actors, critic)
    shared = P.DevicePolicy({k: v[0] for k, v in actors.items()}, critic)
    slices = [P.DevicePolicy({k: v[a] for k, v in actors.items()}, critic) for a in range(A)]
    crit_p = shared.critic_p
    print("forward (actor + critic, sampled) and act (actor, mode):")
    for E in (2048, 65536):
        g = torch.Generator(device=dev).manual_seed(1)
        xs, xo, xc = torch.randn(E, A, D, device=dev, generator=g), torch.randn(E, A, A - 1, 3, device=dev, generator=g), torch.randn(E, A, K, 5, device=dev, generator=g)

        fwd = {"per-agent": lambda: per.forward(xs, xo, xc), "shared": lambda: shared.forward(xs, xo, xc)}
        act = {"per-agent": lambda: per.act(xs, xo, xc), "shared": lambda: shared.act(xs, xo, xc)}
        if not args.only_device:
            # A calls of the shared policy, each on the whole observation (an [E, 1, ...] slice has A - 1 others the one-agent network has no
            # embedding layout for): the user keeps agent a's rows of call a
            fwd["slices"] = lambda: [pol.forward(xs, xo, xc) for pol in slices]
            act["slices"] = lambda: [pol.act(xs, xo, xc) for pol in slices]
            fwd["torch"] = lambda: [P.torch_forward(P.agent_slice(per.actor_p, a), crit_p, xs.unsqueeze(2), xo, xc) for a in range(A)]
        with torch.no_grad():
            report(f"E={E:6d} forward", alternate(fwd, args.blocks, args.calls), "shared")
            report(f"E={E:6d} act    ", alternate(act, args.blocks, args.calls), "shared")

    print("one minibatch of the actor's update (gradient call + clipped Adam):")
    for envs, steps, mb in ((2048, 64, 16),) + (() if args.skip_large else ((65536, 64, 16),)):
        S = envs * steps
        B = S // mb
        g = torch.Generator(device=dev).manual_seed(2)
        r = lambda *s: torch.randn(*s, device=dev, generator=g)                              # noqa: E731
        xs, xo, xc = r(envs, steps, A, D) * 0.7, r(envs, steps, A, A - 1, 3) * 0.5, r(envs, steps, A, K, 5) * 0.5
        action, adv = r(envs, steps, A, 4), r(envs, steps, A, 1)
        idx = torch.randperm(S, device=dev, generator=g)[:B]
        pa = {k: nn.Parameter(v.clone()) for k, v in actors.items()}
        ps = {k: nn.Parameter(v[0].clone()) for k, v in actors.items()}
        pt = {k: nn.Parameter(v.clone()) for k, v in actors.items()}
        first = AT.policy_loss_and_grad_per_agent(pa, xs, xo, xc, action, torch.zeros(envs, steps, A, 1, device=dev), adv, idx, check_index=False)
        lpo = torch.zeros(S, A, 1, device=dev)
        lpo[idx] = first.log_probs + r(B, A, 1) * 0.15             # timing data: ratios inside the clip and on both sides of it
        lpo = lpo.reshape(envs, steps, A, 1)
        oa, os_ = AT.make_optimizer_per_agent(pa), AT.make_optimizer(ps)
        ot = torch.optim.Adam(pt.values(), lr=5e-4)
        tp = P.parse_parameters_per_agent(pt)[0]

        def torch_step():
            res = AT._torch_loss_and_grad(tp, xs, xo, xc, action, lpo, adv, idx, 0.1, 0.001, per_agent=True)
            nn.utils.clip_grad_norm_(list(tp.values()), 10.0)
            ot.step()
            return res

        fns = {"per-agent": lambda: AT.update_actor_per_agent(pa, xs, xo, xc, action, lpo, adv, oa, index=idx),
               "shared": lambda: AT.update_actor(ps, xs, xo, xc, action, lpo, adv, os_, index=idx)}
        if not args.only_device:
            fns["torch"] = torch_step
        report(f"{B * A:7d} rows", alternate(fns, args.blocks, max(2, args.calls // (6 if B > 100000 else 2))), "shared")
        del xs, xo, xc, action, adv, lpo, pa, ps, pt, oa, os_, ot
        torch.cuda.empty_cache()

    print("one train_rollout at the reference default (2 048 envs x 64 steps, 4 epochs x 16 minibatches, predictor on):")
    import learner_cases as LC
    import per_agent_cases as PC
    from hns_amd import learner
    cfg_s = {**LC.CFG, "ppo_epochs": 4, "num_minibatches": 16}
    cfg_a = {**cfg_s, "share_actor": False}
    st_s, st_a = LC.make_state(A, 3), PC.make_state(A, 3)
    ro = LC.to_device(LC.make_rollout(st_s, 2048, 64, A, 4), dev)
    st_s, st_a = LC.clone_state(st_s, dev), PC.clone_state(st_a, dev)
    Ls = learner.DeviceLearner(st_s["actor"], st_s["critic"], cfg_s, tp_net=st_s["tp"], value_normalizer=st_s["vn"])
    La = learner.PerAgentDeviceLearner(st_a["actor"], st_a["critic"], cfg_a, tp_net=st_a["tp"], value_normalizer=st_a["vn"])
    report("train_rollout", alternate({"per-agent": lambda: La.train_rollout(**ro), "shared": lambda: Ls.train_rollout(**ro)}, args.blocks, 2), "shared")
    print(f"shader clock after: {clock():.0f} MHz")
    probe_env.close()


if __name__ == "__main__":
    main()
