#!/usr/bin/env python3
"""Cost of the GRU op (hns_amd.rnn: hns_gru_forward / hns_gru_backward) against the reference's statements in torch on the same GPU, in the
same process, in alternating blocks:

  (a) op    : rnn.gru forward + .backward() of sum(out dy) + sum(h_last dh)         (one launch forward, three backward)
  (b) torch : modules/rnn.py's flow — a Python loop of nn.GRUCell over the steps, the carried state multiplied by 1 - is_init, torch.stack,
              nn.LayerNorm(output + input), .backward() of the same sum

usage  python tools/gru_cost.py [--blocks 5] [--reps 8] [--only op|torch] [--shapes 1536x16,49152x16,6144x1,196608x1]
Shapes are sequences x steps: 1 536 x 16 is the reference's default minibatch (24 576 rows) as 16-step sequences, 49 152 x 16 the same at
65 536 envs; L = 1 is collection's one-step call and is timed forward only, under no_grad (6 144 = 2 048 envs x 3 agents, 196 608 = 65 536 x 3).
Gradients reach the six parameters, x and h0 on both paths.  `--only op` runs path (a) alone: the run to put under
`rocprofv3 --kernel-trace --stats -- python tools/gru_cost.py --only op` for the four kernels' times."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import hns_amd  # noqa: E402,F401
from hns_amd import rnn as RN  # noqa: E402


class TorchGRU(nn.Module):
    """The reference's statements (modules/rnn.py:44-89) for a [S, L, 128] or [S, 128] input."""

    def __init__(self):
        super().__init__()
        self.cell = nn.GRUCell(128, 128)
        self.layer_norm = nn.LayerNorm(128)

    def forward(self, x, h, is_initial):
        if x.dim() == 3:
            mask = (1 - is_initial.float()).reshape(x.shape[0], x.shape[1], 1)
            output = []
            for i in range(x.shape[1]):
                h = h * mask[:, i]
                h = self.cell(x[:, i], h)
                output.append(h.clone())
            output = torch.stack(output, dim=1)
        else:
            output = h = self.cell(x, h * (1 - is_initial.float()).reshape(x.shape[0], 1))
        return self.layer_norm(output + x), h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--only", choices=("op", "torch"), default=None)
    ap.add_argument("--shapes", default="1536x16,49152x16,6144x1,196608x1")
    a = ap.parse_args()
    dev = torch.device("cuda")
    op = RN.GRU().to(dev)
    ref = TorchGRU().to(dev)
    ref.load_state_dict(op.state_dict())
    g = torch.Generator(device=dev).manual_seed(0)
    for shape in a.shapes.split(","):
        S, L = (int(v) for v in shape.split("x"))
        train = L > 1
        x = torch.randn(*((S, L, 128) if train else (S, 128)), device=dev, generator=g).requires_grad_(train)
        h0 = (0.5 * torch.randn(S, 128, device=dev, generator=g)).requires_grad_(train)
        flags = torch.rand(*((S, L) if train else (S,)), device=dev, generator=g) < 0.05
        dy, dh = torch.randn_like(x), torch.randn_like(h0)

        def step(mod):
            if not train:
                with torch.no_grad():
                    return mod(x, h0, flags)
            for p in (*mod.parameters(), x, h0):
                p.grad = None
            out, h = mod(x, h0, flags)
            if mod is op:
                h = h[:, 0]                                      # (the module pads h to the sequence length, as the reference does)
            torch.autograd.backward([out, h], [dy, dh])

        def timed(mod):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                step(mod)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.reps * 1e3

        paths = {"op": op, "torch": ref}
        if a.only:
            paths = {a.only: paths[a.only]}
        for mod in paths.values():                               # warm-up: allocations, lazy module loads
            for _ in range(3):
                step(mod)
        times = {k: [] for k in paths}
        for _ in range(a.blocks):
            for k, mod in paths.items():
                times[k].append(timed(mod))
        med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
        what = "forward + backward" if train else "forward only (no_grad)"
        print(f"GRU {S} sequences x {L} steps = {S * L} rows, {what}")
        label = {"op": "(a) op        ", "torch": "(b) torch flow"}
        for k, t in times.items():
            print(f"  {label[k]}: median {med[k]:.3f} ms per call   blocks {' '.join(f'{v:.3f}' for v in t)}   spread {min(t):.3f}-{max(t):.3f}")
        if not a.only:
            print(f"  ratio: torch / op {med['torch'] / med['op']:.2f}")
        if train:
            ws = hns_amd.abi.load_library().hns_gru_workspace_bytes(S, L, 1)
            print(f"  kept between the passes: h_hist {S * L * 512 / 1e6:.1f} MB; backward workspace {ws / 1e6:.1f} MB (gate gradients {S * L * 2048 / 1e6:.1f} MB)")
        del x, h0, dy, dh
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
