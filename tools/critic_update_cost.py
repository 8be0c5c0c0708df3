#!/usr/bin/env python3
"""Cost of one critic minibatch update on the device path (hns_critic_train_grad + hns_adam_clipped) against the reference's torch flow
(autograd through the PartialAttentionEncoder restatement, clip_grad_norm_, torch.optim.Adam) on the same GPU, in the same process, in
alternating blocks (as tools/tp_train_cost.py): usage  python tools/critic_update_cost.py [--envs 2048] [--steps 64] [--minibatches 16]
[--blocks 5] [--reps 8].  A minibatch is envs * steps / minibatches env-steps x 3 agents (the reference default: 24 576 rows)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import hns_amd  # noqa: E402,F401
from hns_amd import critic_train as CT  # noqa: E402
from hns_amd import policy as P  # noqa: E402


def torch_update(p, opt, xs, xo, xc, bv, ret, idx, loss_fn):
    """update_critic's statements on the gathered minibatch (mappo.py:326-352)."""
    values = F.linear(P._encoder(p, xs[idx], xo[idx], xc[idx]), p["head_w"], p["head_b"])
    b, r = bv[idx], ret[idx]
    clipped = b + (values - b).clamp(-0.1, 0.1)
    value_loss = torch.max(loss_fn(r, values), loss_fn(r, clipped))
    value_loss.backward()
    norm = nn.utils.clip_grad_norm_(list(p.values()), 10.0)
    opt.step()
    opt.zero_grad(set_to_none=True)
    return value_loss, norm, 1 - F.mse_loss(values, r) / r.var()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--minibatches", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    a = ap.parse_args()
    dev = torch.device("cuda")
    A, K, D = 3, 5, 35
    S = a.envs * a.steps
    B = S // a.minibatches
    g = torch.Generator().manual_seed(0)
    _, critic = P.random_parameters(D, A, 1)
    names = {k: P.CRITIC_NAMES[k] for k in critic}
    dev_p = {k: nn.Parameter(v.to(dev)) for k, v in critic.items()}
    ref_p = {names[k]: nn.Parameter(v.to(dev)) for k, v in critic.items()}
    # the rollout, chunked so that the host never holds it twice
    xs = torch.randn(a.envs, a.steps, A, 1, D, device=dev) * 0.7
    xo = torch.randn(a.envs, a.steps, A, A - 1, 3, device=dev) * 0.5
    xc = torch.randn(a.envs, a.steps, A, K, 5, device=dev) * 0.5
    bv = torch.randn(a.envs, a.steps, A, 1, device=dev) * 0.3
    ret = bv + torch.randn(a.envs, a.steps, A, 1, device=dev)
    fxs, fxo, fxc, fbv, fret = (t.reshape(S, *t.shape[2:]) for t in (xs, xo, xc, bv, ret))
    idx = torch.randperm(S, generator=g)[:B].to(dev)
    od = CT.make_optimizer(dev_p)
    orf = torch.optim.Adam(ref_p.values(), lr=5e-4)
    loss_fn = nn.HuberLoss(delta=10.0)

    def dev_step():
        CT.update_critic(dev_p, xs, xo, xc, bv, ret, od, index=idx, check_index=False)

    def ref_step():
        torch_update(ref_p, orf, fxs, fxo, fxc, fbv, fret, idx, loss_fn)

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
    print(f"critic update, {a.envs} envs x {a.steps} steps / {a.minibatches} minibatches = {B} env-steps x {A} agents = {rows} rows per minibatch")
    print(f"  device path : median {md:.3f} ms per minibatch   blocks {' '.join(f'{t:.3f}' for t in td)}")
    print(f"  torch flow  : median {mr:.3f} ms per minibatch   blocks {' '.join(f'{t:.3f}' for t in tr)}")
    print(f"  ratio torch / device {mr / md:.2f}   (block spread: device {min(td):.3f}-{max(td):.3f}, torch {min(tr):.3f}-{max(tr):.3f})")
    print(f"  matrix work {flops / 1e9:.1f} GFLOP: {flops / md / 1e9:.1f} TF/s = {flops / md / 1e9 / 157.3 * 100:.1f} % of the 157.3 TF f32 matrix peak")
    tiles = (rows + 31) // 32
    stage, part = 12 * rows * 512, 2 * tiles * (2308 + 128 * D) * 4      # the operand pairs; two partial rows of 2 308 + 128 D floats per tile
    print(f"  workspace traffic: staged operand pairs {stage / 1e6:.0f} MB + per-tile partial rows {part / 1e6:.0f} MB, written + read: "
          f"{2 * (stage + part) / md / 1e9 * 1e3 / 8000 * 100:.1f} % of 8 TB/s over the whole update")
    print(f"  a rollout's {4 * a.minibatches} minibatches: device {4 * a.minibatches * md:.1f} ms, torch {4 * a.minibatches * mr:.1f} ms")


if __name__ == "__main__":
    main()
