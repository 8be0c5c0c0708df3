#!/usr/bin/env python3
"""Cost of one critic minibatch update written over the encoder op (hns_amd.encoder) against the fused update and the torch flow, on the same
GPU, in the same process, in alternating blocks (as tools/critic_update_cost.py, at its shapes):

  (a) op    : encode (hns_encoder_forward), a torch nn.Linear(128, 1), the clipped Huber value loss in torch, .backward() (hns_encoder_backward),
              the total norm in torch, hns_adam_clipped (ClippedAdam)
  (b) fused : critic_train.update_critic (hns_critic_train_grad + hns_adam_clipped), which the op does not touch
  (c) torch : autograd through the restatement of the encoder, clip_grad_norm_, torch.optim.Adam

usage  python tools/encoder_cost.py [--envs 2048] [--steps 64] [--minibatches 16] [--blocks 5] [--reps 8] [--only op|fused|torch]
A minibatch is envs * steps / minibatches env-steps x 3 agents: 24 576 rows at the defaults, 786 432 with --envs 65536.  `--only op` runs
path (a) alone: the run to put under `rocprofv3 --kernel-trace --stats -- python tools/encoder_cost.py --only op` for the two tile kernels'
times (hns_critic_kernel<false, 0>, hns_critic_kernel<true, 0>)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import hns_amd  # noqa: E402,F401
from hns_amd import critic_train as CT  # noqa: E402
from hns_amd import encoder as EN  # noqa: E402
from hns_amd import policy as P  # noqa: E402
from critic_update_cost import torch_update  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--minibatches", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--only", choices=("op", "fused", "torch"), default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    A, K, D = 3, 5, 35
    S = a.envs * a.steps
    B = S // a.minibatches
    g = torch.Generator().manual_seed(0)
    _, critic = P.random_parameters(D, A, 1)
    names = {k: P.CRITIC_NAMES[k] for k in critic}
    fused_p = {k: nn.Parameter(v.to(dev)) for k, v in critic.items()}
    torch_p = {names[k]: nn.Parameter(v.to(dev)) for k, v in critic.items()}
    enc = EN.AttentionEncoder.from_reference(critic, "base.").to(dev)
    head = nn.Linear(128, 1).to(dev)
    with torch.no_grad():
        head.weight.copy_(critic["v_out.weight"])
        head.bias.copy_(critic["v_out.bias"])
    op_params = [*enc.parameters(), *head.parameters()]
    xs = torch.randn(a.envs, a.steps, A, 1, D, device=dev) * 0.7
    xo = torch.randn(a.envs, a.steps, A, A - 1, 3, device=dev) * 0.5
    xc = torch.randn(a.envs, a.steps, A, K, 5, device=dev) * 0.5
    bv = torch.randn(a.envs, a.steps, A, 1, device=dev) * 0.3
    ret = bv + torch.randn(a.envs, a.steps, A, 1, device=dev)
    fxs, fxo, fxc, fbv, fret = (t.reshape(S, *t.shape[2:]) for t in (xs, xo, xc, bv, ret))
    idx = torch.randperm(S, generator=g)[:B].to(dev)
    o_op = CT.ClippedAdam(op_params, lr=5e-4, max_grad_norm=10.0)
    o_fused = CT.make_optimizer(fused_p)
    o_torch = torch.optim.Adam(torch_p.values(), lr=5e-4)
    loss_fn = nn.HuberLoss(delta=10.0)
    lib = hns_amd.abi.load_library()
    ws = torch.empty(lib.hns_encoder_workspace_bytes(B * A, D, A, K, 1), dtype=torch.uint8, device=dev)

    def op_step():
        values = head(enc(xs, xo, xc, idx, workspace=ws, check_index=False))
        b, r = fbv[idx], fret[idx]
        clipped = b + (values - b).clamp(-0.1, 0.1)
        value_loss = torch.max(loss_fn(r, values), loss_fn(r, clipped))
        for p in op_params:
            p.grad = None
        value_loss.backward()
        norm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm([p.grad for p in op_params])))
        o_op.step(grad_norm=norm)

    def fused_step():
        CT.update_critic(fused_p, xs, xo, xc, bv, ret, o_fused, index=idx, check_index=False)

    def torch_step():
        torch_update(torch_p, o_torch, fxs, fxo, fxc, fbv, fret, idx, loss_fn)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e3

    paths = {"op": op_step, "fused": fused_step, "torch": torch_step}
    if a.only:
        paths = {a.only: paths[a.only]}
    for fn in paths.values():                                    # warm-up: allocations, lazy module loads
        for _ in range(3):
            fn()
    times = {k: [] for k in paths}
    for _ in range(a.blocks):
        for k, fn in paths.items():
            times[k].append(timed(fn))
    rows = B * A
    med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
    print(f"critic update over the encoder op, {a.envs} envs x {a.steps} steps / {a.minibatches} minibatches = {B} env-steps x {A} agents = {rows} rows per minibatch")
    label = {"op": "(a) op path   ", "fused": "(b) fused path", "torch": "(c) torch flow"}
    for k, t in times.items():
        print(f"  {label[k]}: median {med[k]:.3f} ms per minibatch   blocks {' '.join(f'{x:.3f}' for x in t)}   spread {min(t):.3f}-{max(t):.3f}")
    if not a.only:
        print(f"  ratios: op / fused {med['op'] / med['fused']:.2f}   torch / op {med['torch'] / med['op']:.2f}   torch / fused {med['torch'] / med['fused']:.2f}")
        print(f"  features + d features: {2 * rows * 512 / 1e6:.1f} MB written and {2 * rows * 512 / 1e6:.1f} MB read per update (rows x 512 B each way)")


if __name__ == "__main__":
    main()
