#!/usr/bin/env python3
"""Generate tests/golden/g_gru.npz by EXECUTING the reference's GRU (authoring container only: needs the reference checkout; never run on the GPU
box, never from tests).

The reference's own class (omni_drones/learning/modules/rnn.py::GRU, imported from the checkout by path: the file imports torch alone) with
input_size = hidden_size = 128, as make_critic / make_actor build it behind the encoder, on CPU fp32 with one thread.  Its LayerNorm's
parameters and the cell's biases are perturbed (0.1 N(0, 1)) so that no term drops out.  Two cases:
  seq   x [5, 3, 128] with h [5, 128] and is_initial [5, 3, 1] (flags at several steps, one at t = 0)
  step  x [33, 128] with h [33, 128] and is_initial [33, 1]: the one-step call of collection
Stored per case: x, h0, is_init, out, h (the state after the last step: the reference pads it to the sequence length, every copy is the same),
and the gradients of a seeded (out * dy).sum() + (h * dh).sum() with respect to the six parameters, x and h0, with dy and dh themselves.  The
parameters are stored once (bfloat16 values); of the two weight gradients every eighth row is stored (rows of all three gates)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as M  # noqa: E402

RNN = "omni_drones/learning/modules/rnn.py"
ROWS = 8
NAMES = ("cell.weight_ih", "cell.weight_hh", "cell.bias_ih", "cell.bias_hh", "layer_norm.weight", "layer_norm.bias")


def main():
    torch.set_num_threads(1)
    torch.manual_seed(20261019)
    GRU = M.load_by_path("ref_rnn", RNN).GRU
    net = GRU(128, 128)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, t in net.named_parameters():
            if not n.startswith("cell.weight"):
                t.add_(0.1 * torch.randn(t.shape, generator=g))
            t.copy_(t.to(torch.bfloat16).float())               # 8 significant bits: the file stays small, the network runs on these values
    assert tuple(n for n, _ in net.named_parameters()) == NAMES
    out = {"param:" + n: t.detach().numpy().copy() for n, t in net.named_parameters()}
    for tag, shape in (("seq", (5, 3, 128)), ("step", (33, 128))):
        S = shape[0]
        x = torch.randn(*shape, generator=g).requires_grad_(True)
        h0 = (0.5 * torch.randn(S, 128, generator=g)).requires_grad_(True)
        flags = torch.rand(*shape[:-1], 1, generator=g) < 0.3
        flags[0, ..., 0] = True if len(shape) == 2 else torch.tensor([True, False, True])
        y, h = net(x, h0, flags)
        if len(shape) == 3:
            assert all(torch.equal(h[:, 0], h[:, t]) for t in range(shape[1]))
            h = h[:, 0]
        dy, dh = torch.randn(y.shape, generator=g), torch.randn(h.shape, generator=g)
        net.zero_grad()
        ((y * dy).sum() + (h * dh).sum()).backward()
        out.update({f"{tag}:x": x.detach().numpy(), f"{tag}:h0": h0.detach().numpy(), f"{tag}:is_init": flags[..., 0].numpy(),
                    f"{tag}:out": y.detach().numpy(), f"{tag}:h": h.detach().numpy(), f"{tag}:dy": dy.numpy(), f"{tag}:dh": dh.numpy(),
                    f"{tag}:grad:x": x.grad.numpy().copy(), f"{tag}:grad:h0": h0.grad.numpy().copy()})
        for n, t in net.named_parameters():
            out[f"{tag}:grad:{n}"] = t.grad.numpy()[::ROWS].copy() if n.startswith("cell.weight") else t.grad.numpy().copy()
        assert flags.any() and not flags.all()
    path = os.path.join(M.OUT, "g_gru.npz")
    np.savez_compressed(path, cases=np.array(["seq", "step"]), **out)
    print(f"g_gru: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
