#!/usr/bin/env python3
"""Cost of training recurrent per-agent actors on the device (share_actor: False with actor.rnn; hns_amd.rnn_train.update_actor_rnn_per_agent,
learner.PerAgentRecurrentDeviceLearner) against what it stands beside, at 3v1, K = 5, D = 35, L = 16, on a synthetic stored
rollout, in alternating blocks of ONE process (tools/per_agent_rnn_cost.py's method: every arm warmed, wall clock around a block with a
device synchronisation at both ends, so the host's share counts):

  one actor minibatch at 24 576 rows (512 segments) and 786 432 rows (16 384 segments), cached workspace, bucket and optimiser:
      per-agent   rnn_train.update_actor_rnn_per_agent on the stacked tensors
      shared      rnn_train.update_actor_rnn at the same shape (the floor: the same tiles and FLOPs, one set of weights)
      torch       the reference's torch flow with per-agent modules on the same GPU: policy_train.encoder, the GRU as an nn.GRUCell-style loop
                  (rnn.restatement) and a DiagGaussian head per agent's slice under autograd, the loss over all rows, clip_grad_norm_,
                  torch.optim.Adam over the 29 stacked tensors
  one train_rollout at the reference default (2 048 envs x 64 steps, 16 minibatches, 4 epochs, predictor off):
      per-agent   PerAgentRecurrentDeviceLearner        shared   RecurrentDeviceLearner

    python tools/per_agent_rnn_update_cost.py [--blocks 5] [--calls 10] [--skip-torch] [--skip-learner]
    python tools/per_agent_rnn_update_cost.py --existing LABEL    # the shared paths alone, one line (alternating processes, two trees)
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/per_agent_rnn_update_cost.py --trace (a run of its own)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import hns_amd  # noqa: E402,F401
from hns_amd import learner, rnn, rnn_train  # noqa: E402
from hns_amd import policy as P  # noqa: E402
from hns_amd import policy_train as PT  # noqa: E402

A, K, D, L = 3, 5, 35, 16


def alternate(fns, blocks, calls):
    """{name: sorted ms per call over the blocks}: every function warmed, then blocks of `calls` calls in turn."""
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
        print(f"  {what} {k:10s} median {med[k]:10.3f} ms  (min {v[0]:.3f}, max {v[-1]:.3f})  x{med[k] / med[base]:.3f} of {base}", flush=True)
    return med


def networks(dev, seed=0):
    """(the shared recurrent actor, the stacked one, the shared recurrent critic) under the reference's names, on `dev`."""
    actor, critic = P.random_parameters(D, A, seed)
    actor.update(P.random_rnn_parameters(seed + 1))
    critic.update(P.random_rnn_parameters(seed + 2))
    actors, _ = P.random_parameters_per_agent(D, A, seed)
    actors.update(P.random_rnn_parameters_per_agent(A, seed + 1))
    to = lambda p: {k: v.to(dev).contiguous() for k, v in p.items()}           # noqa: E731
    return to(actor), to(actors), to(critic)


def rollout(N, T, dev, seed=1):
    """A synthetic stored rollout [N, T]: learner_kwargs and recurrent_kwargs (log_probs near the policy's own: the ratios stay near 1)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)      # noqa: E731
    kw = {"obs_self": r(N, T, A, 1, D) * 0.7, "obs_others": r(N, T, A, A - 1, 3) * 0.5, "obs_cylinders": r(N, T, A, K, 5) * 0.5,
          "action": r(N, T, A, 4) * 0.5, "log_probs": r(N, T, A, 1) * 0.05 - 3.9, "state_value": r(N, T, A, 1) * 0.3,
          "next_obs_last": (r(N, A, 1, D) * 0.7, r(N, A, A - 1, 3) * 0.5, r(N, A, K, 5) * 0.5), "reward": r(N, T, A, 1),
          "done": torch.rand(N, T, 1, device=dev, generator=g) < 0.02, "agent_done": None, "tp": None}
    rk = {"is_init": torch.rand(N, T, 1, device=dev, generator=g) < 0.02, "actor_rnn_state": r(N, T // L, A, 128) * 0.5,
          "critic_rnn_state": r(N, T // L, A, 128) * 0.5, "rnn_seq_len": L, "last_critic_rnn_state": r(N, A, 128) * 0.5,
          "last_is_init": torch.rand(N, 1, device=dev, generator=g) < 0.02}
    return kw, rk


def torch_update(actors, kw, rk, seg, opt):
    """The reference's torch flow on one minibatch with per-agent modules: update_actor's statements (mappo.py:281-318) under autograd."""
    net = rnn_train.network_parameters(actors, True, stacked=True)
    B = seg.numel()
    idx = rnn_train._step_index(seg, L)
    flat = lambda t: t.reshape(-1, *t.shape[2:])[idx]            # noqa: E731
    xs, xo, xc = flat(kw["obs_self"]), flat(kw["obs_others"]), flat(kw["obs_cylinders"])
    h0 = rk["actor_rnn_state"].reshape(-1, A, 128)[seg]
    flags = rk["is_init"].reshape(-1, L)[seg].float()
    act, lpo, adv = flat(kw["action"]).reshape(B, L, A, 4), flat(kw["log_probs"]).reshape(B, L, A, 1), flat(kw["reward"]).reshape(B, L, A, 1)
    logp, ent = [], []
    for a in range(A):
        x = PT.encoder(P.agent_slice(net.encoder, a), xs[:, a], xo[:, a], xc[:, a]).reshape(B, L, 128)
        y, _ = rnn.restatement(P.agent_slice(net.gru, a), x, h0[:, a], flags)
        mean = y @ net.head["head_w"][a].t() + net.head["head_b"][a]
        dist = torch.distributions.Independent(torch.distributions.Normal(mean, torch.exp(net.head["log_std"][a]).expand_as(mean)), 1)
        logp.append(dist.log_prob(act[:, :, a]))
        ent.append(dist.entropy())
    ratio = torch.exp(torch.stack(logp, 2).unsqueeze(-1) - lpo)
    loss = -torch.mean(torch.min(ratio * adv, ratio.clamp(0.9, 1.1) * adv) * 4) - 1e-3 * torch.stack(ent, 2).mean()
    opt.zero_grad(set_to_none=True)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(opt.param_groups[0]["params"], 10.0)
    opt.step()


def minibatch_arms(dev, B, with_torch, with_per_agent=True):
    """{arm: a function that runs one actor minibatch of B segments} on a rollout of B envs x 16 steps."""
    actor, actors, critic = networks(dev)
    kw, rk = rollout(B, L, dev)
    seg = torch.randperm(B, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    args = (kw["obs_self"], kw["obs_others"], kw["obs_cylinders"], rk["actor_rnn_state"], rk["is_init"], kw["action"], kw["log_probs"], kw["reward"])
    fns = {}

    def arm(fn, net, stacked):
        opt = rnn_train.make_optimizer(net, {"share_actor": False} if stacked else None, actor=True, **({"stacked": True} if stacked else {}))
        bucket = rnn_train.make_bucket(net, True, **({"stacked": True} if stacked else {}))
        ws, out = rnn_train.RnnWorkspace(), torch.empty(4, device=dev)
        return lambda: fn(net, *args, opt, segment=seg, seq_len=L, workspace=ws, out=out, bucket=bucket)

    if with_per_agent:
        fns["per-agent"] = arm(rnn_train.update_actor_rnn_per_agent, actors, True)
    fns["shared"] = arm(rnn_train.update_actor_rnn, actor, False)
    if with_torch:
        leaves = {k: v.clone().requires_grad_(True) for k, v in actors.items()}
        topt = torch.optim.Adam(list(leaves.values()), lr=5e-4)
        fns["torch"] = lambda: torch_update(leaves, kw, rk, seg, topt)
    cargs = (kw["obs_self"], kw["obs_others"], kw["obs_cylinders"], rk["critic_rnn_state"], rk["is_init"], kw["state_value"], kw["reward"])
    copt, cws, cout = rnn_train.make_optimizer(critic, None, actor=False), rnn_train.RnnWorkspace(), torch.empty(3, device=dev)
    cbucket = rnn_train.make_bucket(critic, False)
    critic_fn = lambda: rnn_train.update_critic_rnn(critic, *cargs, copt, segment=seg, seq_len=L, workspace=cws, out=cout, bucket=cbucket)   # noqa: E731
    return fns, critic_fn


CFG = {"ppo_epochs": 4, "num_minibatches": 16, "use_TP_net": 0, "actor": {"rnn": {"train_seq_len": L}}, "critic": {"rnn": {"train_seq_len": L}}}


def learner_arms(dev, with_per_agent=True):
    actor, actors, critic = networks(dev)
    kw, rk = rollout(2048, 64, dev)
    vn = lambda: learner.ValueNorm1().to(dev)                    # noqa: E731
    fns = {}
    if with_per_agent:
        per = learner.PerAgentRecurrentDeviceLearner(actors, {k: v.clone() for k, v in critic.items()}, {**CFG, "share_actor": False}, value_normalizer=vn())
        fns["per-agent"] = lambda: per.train_rollout(**kw, **rk)
    sh = learner.RecurrentDeviceLearner(actor, critic, CFG, value_normalizer=vn())
    fns["shared"] = lambda: sh.train_rollout(**kw, **rk)
    return fns


def existing(label, blocks, calls):
    """The paths that existed before: update_actor_rnn and update_critic_rnn at 24 576 rows and RecurrentDeviceLearner.train_rollout at the
    reference default, medians; run from a tree's own copy of this file, so each process measures its own tree's Python and library."""
    dev = torch.device("cuda")
    fns, critic_fn = minibatch_arms(dev, 512, False, with_per_agent=False)
    t = alternate({"actor": fns["shared"], "critic": critic_fn}, blocks, calls)
    lt = alternate(learner_arms(dev, with_per_agent=False), max(3, blocks // 2), 1)
    med = lambda v: v[len(v) // 2]                               # noqa: E731
    print(f"{label} update_actor_rnn_ms {med(t['actor']):.4f} update_critic_rnn_ms {med(t['critic']):.4f} train_rollout_ms {med(lt['shared']):.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-learner", action="store_true")
    ap.add_argument("--trace", action="store_true", help="a few per-agent and shared minibatches at both sizes and nothing else: run under a kernel trace")
    ap.add_argument("--existing", metavar="LABEL", help="the shared paths alone, one line")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("per_agent_rnn_update_cost: no GPU — nothing is measured without one")
    if args.existing:
        return existing(args.existing, args.blocks, args.calls)
    dev = torch.device("cuda")
    print("one actor minibatch (3v1, K 5, D 35, L 16), cached workspace, bucket and optimiser:")
    for B in (512, 16384):
        fns, _ = minibatch_arms(dev, B, not (args.skip_torch or args.trace))
        if args.trace:
            for _ in range(3):
                for f in fns.values():
                    f()
            torch.cuda.synchronize()
        else:
            report(f"rows={B * L * A:7d}", alternate(fns, args.blocks, args.calls if B == 512 else max(2, args.calls // 5)), "shared")
        del fns
        torch.cuda.empty_cache()
    if not (args.skip_learner or args.trace):
        print("one train_rollout at 2 048 envs x 64 steps (4 epochs x 16 minibatches of 512 segments, predictor off):")
        report("train_rollout", alternate(learner_arms(dev), max(3, args.blocks // 2 + 1), 1), "shared")


if __name__ == "__main__":
    main()
