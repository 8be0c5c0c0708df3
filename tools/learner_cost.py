#!/usr/bin/env python3
"""Cost of one MAPPOPolicy.train_op per rollout, three arms on the same GPU in alternating blocks of one process (as tools/policy_cost.py):
  (a) learner   DeviceLearner.train_rollout: cached workspaces, scalars into the info table, one copy to the host
  (b) hand      the same blocks through the package's public functions as a pasted-in mappo.py calls them: per-call workspaces, the
                per-minibatch .item()s of update_actor / update_critic, the torch statements of the info row
  (c) torch     the reference's torch flow on device tensors, as tools/actor_update_cost.py and tools/critic_update_cost.py define it (the
                modules' CPU-path statements: the GAE loop over T, autograd through the encoder restatement, clip_grad_norm_, torch.optim.Adam)
usage  python tools/learner_cost.py [--envs 2048] [--steps 64] [--minibatches 16] [--epochs 4] [--blocks 3] [--reps 2] [--arms learner,hand,torch]
The reference default: 2 048 envs x 64 steps x 3 agents, K = 5, D = 35, 4 epochs x 16 minibatches, the predictor on."""
import argparse
import copy
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import hns_amd  # noqa: E402,F401
from hns_amd import actor_train as AT  # noqa: E402
from hns_amd import critic_train as CT  # noqa: E402
from hns_amd import gae, learner, tp_train  # noqa: E402
from hns_amd import policy as P  # noqa: E402
from hns_amd import policy_train as PT  # noqa: E402
from hns_amd.tp_net import TPNet  # noqa: E402

A, K, D, HIST, FUTURE = 3, 5, 35, 10, 5


def make_state(dev, cfg):
    actor, critic = P.random_parameters(D, A, 1)
    torch.manual_seed(2)
    s = {"actor": {k: nn.Parameter(v.to(dev)) for k, v in actor.items()}, "critic": {k: nn.Parameter(v.to(dev)) for k, v in critic.items()},
         "tp": TPNet(7 + 3 * A, 3 * FUTURE, FUTURE, 1).to(dev), "vn": learner.ValueNorm1().to(dev)}
    return s


def make_rollout(dev, N, T, state):
    g = torch.Generator(device=dev).manual_seed(3)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)                                # noqa: E731
    xs, xo, xc = r(N, T, A, 1, D) * 0.7, r(N, T, A, A - 1, 3) * 0.5, r(N, T, A, K, 5) * 0.5
    pol = P.DevicePolicy(state["actor"], state["critic"])
    out = pol.forward(xs.reshape(N * T, A, 1, D), xo.reshape(N * T, A, A - 1, 3), xc.reshape(N * T, A, K, 5))
    return {"obs_self": xs, "obs_others": xo, "obs_cylinders": xc, "action": out.action.reshape(N, T, A, 4), "log_probs": out.log_prob.reshape(N, T, A, 1),
            "state_value": out.value.reshape(N, T, A, 1), "next_obs_last": (r(N, A, 1, D) * 0.7, r(N, A, A - 1, 3) * 0.5, r(N, A, K, 5) * 0.5),
            "reward": r(N, T, A, 1), "done": torch.rand(N, T, 1, device=dev, generator=g) < 0.01, "agent_done": None,
            "tp": (r(N, T, HIST, 7 + 3 * A) * 0.5, torch.rand(N, T, 3, device=dev, generator=g) * 2 - 1, torch.ones(N, T, 1, device=dev))}


def hand_arm(state, cfg):
    """(b): what INTEGRATION.md's three paste-in recipes amount to inside the reference's train_op."""
    oa, oc = AT.make_optimizer(state["actor"], cfg), CT.make_optimizer(state["critic"], cfg)
    ot = tp_train.TPAdam(tp_train.parameters(state["tp"]), lr=1e-4)
    pol = P.DevicePolicy(state["actor"], state["critic"], cfg)

    def run(ro):
        N, T = ro["action"].shape[:2]
        next_value = pol.forward(*ro["next_obs_last"], value_only=True).value
        adv, ret, _, (m, s) = gae.rollout_targets(ro["reward"], ro["done"].unsqueeze(-1), ro["state_value"], next_value, cfg["gamma"], cfg["gae_lambda"],
                                                  value_normalizer=state["vn"], return_moments=True)
        info = {"TP_loss": tp_train.update_tp(state["tp"], *ro["tp"], FUTURE, 1, cfg["num_minibatches"], cfg["TP_epochs"], ot).item()}
        rows = []
        for _ in range(cfg["ppo_epochs"]):
            for idx in tp_train.minibatches(N * T, cfg["num_minibatches"], adv.device):
                sa = AT.update_actor(state["actor"], ro["obs_self"], ro["obs_others"], ro["obs_cylinders"], ro["action"], ro["log_probs"], adv, oa, index=idx, cfg=cfg)
                sc = CT.update_critic(state["critic"], ro["obs_self"], ro["obs_others"], ro["obs_cylinders"], ro["state_value"], ret, oc, index=idx, cfg=cfg)
                rows.append({k: v.item() for k, v in {**sa, **sc}.items()})          # mappo.py:319-324, :348-352: an .item() per scalar
        info.update({k: sum(r[k] for r in rows) / len(rows) for k in rows[0]})
        info["advantages_mean"], info["advantages_std"] = m.item(), s.item()
        info["action_norm"] = ro["action"].norm(dim=-1).mean().item()
        info["value_running_mean"] = state["vn"].running_mean.mean().item()
        return info
    return run


def torch_arm(state, cfg):
    """(c): the torch statements throughout, on device tensors."""
    pa, pc = AT.actor_parameters(state["actor"]), CT.critic_parameters(state["critic"])
    oa, oc = torch.optim.Adam(pa.values(), lr=5e-4), torch.optim.Adam(pc.values(), lr=5e-4)
    ot = torch.optim.Adam(state["tp"].parameters(), lr=1e-4)
    vn = state["vn"]

    def run(ro):
        N, T = ro["action"].shape[:2]
        xs, xo, xc = PT.as_rollout(ro["obs_self"], ro["obs_others"], ro["obs_cylinders"])
        with torch.no_grad():
            l = ro["next_obs_last"]
            next_value = P.torch_forward(pa, pc, l[0], l[1], l[2], value_only=True).value
            mean, var = vn.running_mean_var()
            values, next_value = ro["state_value"] * torch.sqrt(var) + mean, next_value * torch.sqrt(var) + mean
            dones = ro["done"].unsqueeze(-1).expand(N, T, A, 1)
            adv, ret = gae._torch_gae(ro["reward"], dones, values, next_value, cfg["gamma"], cfg["gae_lambda"], False)
            m, s = adv.mean(), adv.std()
            adv = (adv - m) / (s + 1e-8)
            w = vn.beta
            vn.running_mean.mul_(w).add_(ret.mean() * (1.0 - w))
            vn.running_mean_sq.mul_(w).add_((ret ** 2).mean() * (1.0 - w))
            vn.debiasing_term.mul_(w).add_(1.0 * (1.0 - w))
            mean, var = vn.running_mean_var()
            ret = (ret - mean) / torch.sqrt(var)
        x, y = tp_train.select_windows(*ro["tp"], FUTURE, 1)
        x4 = tp_train._as_blocks(x)
        tpl = []
        for _ in range(cfg["TP_epochs"]):
            for idx in tp_train.minibatches(x4.shape[0] * x4.shape[1], cfg["num_minibatches"], x.device):
                tpl.append(tp_train._torch_loss_and_grad(state["tp"], x4, y, idx).item())
                ot.step()
        rows = []
        for _ in range(cfg["ppo_epochs"]):
            for idx in tp_train.minibatches(N * T, cfg["num_minibatches"], adv.device):
                a = AT._torch_loss_and_grad(pa, xs, xo, xc, ro["action"], ro["log_probs"], adv, idx, cfg["clip_param"], cfg["entropy_coef"])
                na = nn.utils.clip_grad_norm_(list(pa.values()), cfg["max_grad_norm"])
                oa.step()
                c = CT._torch_loss_and_grad(pc, xs, xo, xc, ro["state_value"], ret, idx, cfg["clip_param"], "huber", 10.0)
                nc = nn.utils.clip_grad_norm_(list(pc.values()), cfg["max_grad_norm"])
                oc.step()
                rows.append([a.policy_loss.item(), na.item(), a.entropy.item(), a.ess.item(), c.value_loss.item(), nc.item(), c.explained_var.item()])
        return {"policy_loss": sum(r[0] for r in rows) / len(rows), "TP_loss": sum(tpl) / len(tpl), "advantages_mean": m.item(),
                "action_norm": ro["action"].norm(dim=-1).mean().item()}
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--minibatches", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--arms", default="learner,hand,torch")
    a = ap.parse_args()
    dev = torch.device("cuda")
    cfg = {"ppo_epochs": a.epochs, "num_minibatches": a.minibatches, "TP_epochs": 1, "use_TP_net": 1, "clip_param": 0.1, "entropy_coef": 0.001,
           "gamma": 0.995, "gae_lambda": 0.95, "max_grad_norm": 10.0, "normalize_advantages": True}
    start = make_state(dev, cfg)
    ro = make_rollout(dev, a.envs, a.steps, start)
    arms = {}
    for name in a.arms.split(","):
        st = copy.deepcopy(start)
        if name == "learner":
            L = learner.DeviceLearner(st["actor"], st["critic"], cfg, tp_net=st["tp"], value_normalizer=st["vn"])
            arms[name] = lambda ro, L=L: L.train_rollout(**ro)
        elif name == "hand":
            arms[name] = hand_arm(st, cfg)
        elif name == "torch":
            arms[name] = torch_arm(st, cfg)
        else:
            raise SystemExit(f"unknown arm {name}")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn(ro)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e3

    first = {k: fn(ro) for k, fn in arms.items()}                # warm-up: allocations, lazy module loads; the first call's info rows
    for fn in arms.values():
        fn(ro)
    times = {k: [] for k in arms}
    for _ in range(a.blocks):
        for k, fn in arms.items():
            times[k].append(timed(fn))
    rows = a.envs * a.steps // a.minibatches * A
    print(f"train_op, {a.envs} envs x {a.steps} steps x {A} agents, {a.epochs} epochs x {a.minibatches} minibatches of {rows} rows, predictor on; "
          f"{a.blocks} alternating blocks of {a.reps} calls, wall time per call with a synchronisation at each end")
    med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
    for k, t in times.items():
        print(f"  {k:8s}: median {med[k]:9.2f} ms per train_op   blocks {' '.join(f'{x:.2f}' for x in t)}   spread {min(t):.2f}-{max(t):.2f}")
    if "learner" in med:
        for k in med:
            if k != "learner":
                print(f"  {k} / learner = {med[k] / med['learner']:.3f}")
    print("  first call from the common start (policy_loss, TP_loss, advantages_mean, action_norm):")
    for k, i in first.items():
        g = lambda n: i.get(n, i.get(f"drone/{n}"))              # noqa: E731
        print(f"    {k:8s}: {g('policy_loss'):.6f} {g('TP_loss'):.6f} {g('advantages_mean'):.6f} {g('action_norm'):.6f}")


if __name__ == "__main__":
    main()
