#!/usr/bin/env python3
"""Cost of the predictor's training step (learning/mappo.py:405-441 with update_TP :252-268): the reference's torch flow (nn.LSTM forward, MSE,
autograd backward through MIOpen, torch.optim.Adam, one loss.item() per minibatch) against hns_amd.tp_train.update_tp (hns_tp_train_grad +
hns_tp_adam per minibatch), both on the GPU, in ONE process, alternating timed blocks (hipEvent pairs around one rollout update each).

Shapes: a 64-step rollout of E envs (I = 16, T = 10, F = 5, window_step 1, 16 minibatches, one epoch: cfg/algo/mappo.yaml), E = 2 048 (the
reference default) and 65 536.  FLOPs from the shapes: per sequence and step 2 * 4H (I + H) forward + 2 * 4H (I + 2H) backward (H = 64); the
fraction is FLOPs / time over the 157 TF f32 matrix peak.

    python tools/tp_train_cost.py [--blocks 5]      -> profiles/r08_tp_train_cost.txt
    python tools/tp_train_cost.py --profile         (two HIP rollout updates at 65 536 envs only, for rocprofv3 --kernel-trace --stats)"""
import argparse
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hns_amd  # noqa: E402,F401
from hns_amd import tp_train as TT  # noqa: E402
from hns_amd.tp_net import TPNet  # noqa: E402

PEAK = 157e12
H, I, T, F, STEPS, NMB = 64, 16, 10, 5, 64, 16


def rollout(E, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(E, STEPS, T, I, device=dev, generator=g) * 0.5
    gt = (torch.rand(E, STEPS, 3, device=dev, generator=g) * 2 - 1) * 0.9
    done = torch.ones(E, STEPS, 1, dtype=torch.bool, device=dev)
    return x, gt, done


def torch_flow(net, opt, crit, x, gt, done):
    """mappo.py:405-441 as written: masked_select, make_dataset_naive's gathers, update_TP per minibatch with loss.item()."""
    xs, y = TT.select_windows(x, gt, done, F, 1)
    xs = xs.reshape(-1, T, I)
    infos = []
    for idx in TT.minibatches(xs.shape[0], NMB, x.device):
        out = net(xs[idx])
        loss = crit(out, y[idx].reshape(idx.numel(), -1))
        opt.zero_grad()
        loss.backward()
        opt.step()
        infos.append(loss.item())
    return infos


def flops(E):
    seqs = (E * (STEPS - F) // NMB) * NMB
    return seqs * T * (2 * 4 * H * (I + H) + 2 * 4 * H * (I + 2 * H))


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_tp_train_cost.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    lines = []
    sizes = [65536] if args.profile else [2048, 65536]
    for E in sizes:
        x, gt, done = rollout(E, dev)
        net_h = TPNet(I, 3 * F, F, 1).to(dev)
        net_t = TPNet(I, 3 * F, F, 1).to(dev)
        net_t.load_state_dict(net_h.state_dict())
        opt_h, opt_t = TT.TPAdam(net_h.parameters()), torch.optim.Adam(net_t.parameters(), lr=1e-4)
        crit = nn.MSELoss()
        hip = lambda: TT.update_tp(net_h, x, gt, done, F, 1, NMB, 1, opt_h)          # noqa: E731
        ref = lambda: torch_flow(net_t, opt_t, crit, x, gt, done)                     # noqa: E731
        if args.profile:
            hip()
            torch.cuda.synchronize()
            hip()
            torch.cuda.synchronize()
            print(f"profile run: two HIP rollout updates at {E} envs")
            return
        hip(), ref()                                                                  # warm-up (MIOpen's find, allocator)
        torch.cuda.synchronize()
        th, tt = [], []
        for _ in range(args.blocks):
            th.append(timed(hip))
            tt.append(timed(ref))
        mh, mt = sorted(th)[len(th) // 2], sorted(tt)[len(tt) // 2]
        fl = flops(E)
        lines.append(f"E={E:6d}  sequences/update={(E * (STEPS - F) // NMB) * NMB:8d}  torch {mt:9.3f} ms  hip {mh:9.3f} ms  ratio {mt / mh:6.2f}x  "
                     f"hip {fl / (mh * 1e-3) / 1e12:6.2f} TF = {fl / (mh * 1e-3) / PEAK:.3f} of the f32 matrix peak  "
                     f"(median of {args.blocks} alternating blocks; torch {min(tt):.3f}-{max(tt):.3f}, hip {min(th):.3f}-{max(th):.3f})")
        print(lines[-1], flush=True)
    head = ["# predictor training step per rollout update (mappo.py:405-441): reference torch flow vs hns_amd.tp_train.update_tp",
            f"# I={I} T={T} F={F} steps={STEPS} minibatches={NMB} epochs=1; device {torch.cuda.get_device_name(0)}; tools/tp_train_cost.py"]
    with open(args.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")


if __name__ == "__main__":
    main()
