"""Cost of the MAPPO policy's forward pass: hns_policy_forward (DevicePolicy) against the torch statements MAPPOPolicy.__call__ + value_op run
(hns_amd.policy.torch_forward on the same GPU), in alternating blocks of one process.  Shapes: 3v1, K = 5, D = 35 (the reference default with
the predictor), 2 048 and 65 536 envs.  Kernel time alone: run under `rocprofv3 --kernel-trace --stats -- python tools/policy_cost.py --only-device`.

    python tools/policy_cost.py [--blocks 6] [--calls 50]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hns_amd  # noqa: E402,F401
from hns_amd import policy as P  # noqa: E402

A, K, D = 3, 5, 35
FLOP_ROW = 2 * (2 * 6 * 128 * 128 + 2 * 128 * (D + 3 * (A - 1) + 5 * K) + 2 * 128 * (A + K) * 2) + 2 * 2 * 128 * 5   # both networks, per row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--only-device", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    actor, critic = (dict((k, v.to(dev)) for k, v in p.items()) for p in P.random_parameters(D, A, seed=0))
    pol = P.DevicePolicy(actor, critic)
    ap_, cp_ = pol.actor_p, pol.critic_p
    print(f"FLOP per row (single-query algebra, both networks): {FLOP_ROW / 1e6:.3f} M;  weight bytes streamed per workgroup of 32 rows: "
          f"{2 * 6 * 128 * 128 * 4 / 1e6:.2f} MB (+ embeddings)")
    for E in (2048, 65536):
        g = torch.Generator(device=dev).manual_seed(1)
        xs = torch.randn(E, A, 1, D, device=dev, generator=g)
        xo = torch.randn(E, A, A - 1, 3, device=dev, generator=g)
        xc = torch.randn(E, A, K, 5, device=dev, generator=g)
        fns = {"device": lambda: pol.forward(xs, xo, xc)}
        if not args.only_device:
            fns["torch"] = lambda: P.torch_forward(ap_, cp_, xs, xo, xc)
        times = {k: [] for k in fns}
        with torch.no_grad():
            for k in fns:
                fns[k]()
            torch.cuda.synchronize()
            for b in range(args.blocks):
                for k, f in fns.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(args.calls):
                        f()
                    e.record()
                    torch.cuda.synchronize()
                    times[k].append(s.elapsed_time(e) / args.calls)
        rows = E * A
        for k, t in times.items():
            t = sorted(t)
            med = t[len(t) // 2]
            print(f"E={E:6d} rows={rows:7d} {k:7s} median {med * 1e3:9.1f} us per call (min {t[0] * 1e3:.1f}, max {t[-1] * 1e3:.1f})  "
                  f"{FLOP_ROW * rows / (med * 1e-3) / 1e12:.2f} TFLOP/s = {FLOP_ROW * rows / (med * 1e-3) / 157.3e12:.3f} of the f32 matrix peak")
        if "torch" in times:
            print(f"E={E:6d} torch / device = {sorted(times['torch'])[args.blocks // 2] / sorted(times['device'])[args.blocks // 2]:.2f}x")


if __name__ == "__main__":
    main()
