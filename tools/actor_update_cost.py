#!/usr/bin/env python3
"""Cost of one actor minibatch update on the device path (hns_actor_train_grad + hns_adam_clipped) against the reference's torch flow
(update_actor's statements as hns_amd.actor_train's CPU path writes them, on device tensors: autograd through the PartialAttentionEncoder
restatement, clip_grad_norm_, torch.optim.Adam) on the same GPU, in the same process, in alternating blocks (as
tools/critic_update_cost.py): usage  python tools/actor_update_cost.py [--envs 2048] [--steps 64] [--minibatches 16] [--blocks 5]
[--reps 8].  A minibatch is envs * steps / minibatches env-steps x 3 agents (the reference default: 24 576 rows)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributions as D  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import hns_amd  # noqa: E402,F401
from hns_amd import actor_train as AT  # noqa: E402
from hns_amd import policy as P  # noqa: E402
from hns_amd import policy_train as PT  # noqa: E402


def torch_update(p, opt, xs, xo, xc, act, lpo, adv, idx):
    """update_actor's statements on the gathered minibatch (mappo.py:271-324; actor_train._torch_loss_and_grad's, with backward() into .grad)."""
    mean = F.linear(PT.encoder(p, xs[idx], xo[idx], xc[idx]), p["head_w"], p["head_b"])
    dist = D.Independent(D.Normal(mean, torch.broadcast_to(torch.exp(p["log_std"]), mean.shape), validate_args=False), 1, validate_args=False)
    logp = dist.log_prob(act[idx]).unsqueeze(-1)
    ent = dist.entropy().unsqueeze(-1)
    a = adv[idx]
    ratio = torch.exp(logp - lpo[idx])
    policy_loss = - torch.mean(torch.min(ratio * a, torch.clamp(ratio, 0.9, 1.1) * a) * 4)
    entropy_loss = - torch.mean(ent)
    opt.zero_grad()
    (policy_loss + entropy_loss * 0.001).backward()
    norm = nn.utils.clip_grad_norm_(list(p.values()), 10.0)
    opt.step()
    ess = (2 * ratio.logsumexp(0) - (2 * ratio).logsumexp(0)).exp().mean() / ratio.shape[0]
    return policy_loss, norm, -entropy_loss, ess


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--minibatches", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    a = ap.parse_args()
    dev = torch.device("cuda")
    A, K, Dm = 3, 5, 35
    S = a.envs * a.steps
    B = S // a.minibatches
    g = torch.Generator().manual_seed(0)
    actor, _ = P.random_parameters(Dm, A, 1)
    dev_p = {k: nn.Parameter(v.to(dev)) for k, v in actor.items()}
    ref_p = {P.ACTOR_NAMES[k]: nn.Parameter(v.to(dev)) for k, v in actor.items()}
    xs = torch.randn(a.envs, a.steps, A, 1, Dm, device=dev) * 0.7
    xo = torch.randn(a.envs, a.steps, A, A - 1, 3, device=dev) * 0.5
    xc = torch.randn(a.envs, a.steps, A, K, 5, device=dev) * 0.5
    act = torch.randn(a.envs, a.steps, A, 4, device=dev)
    adv = torch.randn(a.envs, a.steps, A, 1, device=dev)
    fxs, fxo, fxc, fact, fadv = (t.reshape(S, *t.shape[2:]) for t in (xs, xo, xc, act, adv))
    idx = torch.randperm(S, generator=g)[:B].to(dev)
    # old log-probabilities near the new ones (the device's own from ONE un-timed call with zeros in their place, plus noise): ratios inside the
    # clip and on both sides of it.  Timing data only: nothing keeps a ratio away from the clip's bounds, so these are no inputs for an accuracy
    # comparison (tests/test_hip_actor_train.py builds those)
    out = AT.policy_loss_and_grad(dev_p, xs, xo, xc, act, torch.zeros(a.envs, a.steps, A, 1, device=dev), adv, idx, check_index=False)
    lpo = torch.zeros(S, A, 1, device=dev)
    lpo[idx] = out.log_probs + torch.randn(B, A, 1, device=dev) * 0.15
    for v in dev_p.values():
        v.grad = None
    rlpo = lpo.reshape(a.envs, a.steps, A, 1)
    od = AT.make_optimizer(dev_p)
    orf = torch.optim.Adam(ref_p.values(), lr=5e-4)

    def dev_step():
        AT.update_actor(dev_p, xs, xo, xc, act, rlpo, adv, od, index=idx, check_index=False)

    def ref_step():
        torch_update(ref_p, orf, fxs, fxo, fxc, fact, lpo, fadv, idx)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e3

    for fn in (dev_step, ref_step):                              # warm-up: allocations, lazy module loads
        for _ in range(3):
            fn()
    td, tr = [], []
    for _ in range(a.blocks):
        td.append(timed(dev_step))
        tr.append(timed(ref_step))
    rows = B * A
    flops = rows * 18 * 2 * 128 * 128                            # 6 forward + 6 backward-data + 6 weight-gradient 128 x 128 products per row
    md, mr = sorted(td)[len(td) // 2], sorted(tr)[len(tr) // 2]
    print(f"actor update, {a.envs} envs x {a.steps} steps / {a.minibatches} minibatches = {B} env-steps x {A} agents = {rows} rows per minibatch")
    print(f"  device path : median {md:.3f} ms per minibatch   blocks {' '.join(f'{t:.3f}' for t in td)}")
    print(f"  torch flow  : median {mr:.3f} ms per minibatch   blocks {' '.join(f'{t:.3f}' for t in tr)}")
    print(f"  ratio torch / device {mr / md:.2f}   (block spread: device {min(td):.3f}-{max(td):.3f}, torch {min(tr):.3f}-{max(tr):.3f})")
    print(f"  matrix work {flops / 1e9:.1f} GFLOP: {flops / md / 1e9:.1f} TF/s = {flops / md / 1e9 / 157.3 * 100:.1f} % of the 157.3 TF f32 matrix peak")
    print(f"  a rollout's {4 * a.minibatches} minibatches: device {4 * a.minibatches * md:.1f} ms, torch {4 * a.minibatches * mr:.1f} ms")


if __name__ == "__main__":
    main()
