#!/usr/bin/env python3
"""Generate tests/golden/g_policy_central.npz by EXECUTING the reference's centralised critic (authoring container only: needs the reference
checkout; never run on the GPU box, never from tests).  Reuses make_golden_policy.py's loaders without changing that file.

The reference's own SplitEmbedding, PartialAttentionEncoder (learning/modules/networks.py:125-163, :250-313) and Critic (learning/mappo.py:630-660)
run on CPU in fp32, built as make_critic(..., centralized=True) builds them (mappo.py:553-566) over HideAndSeek's STATE CompositeSpec
(hideandseek.py:343-356: state_drones (A, D), cylinders (K, 5)): v_out = Linear(128, A), orthogonal with gain 0.01, output_shape (A, 1).
The cylinders are fed as the spec declares them, [B, K, 5] (the env's own tensor is [B, A, K, 5], which SplitEmbedding's torch.cat refuses:
DESIGN.md §7.20).  As in g_policy.npz the biases and LayerNorm affine parameters are perturbed, every parameter is rounded to bfloat16 and
stored as its 16 bits, and a later case takes the first case's parameters wherever the shapes agree ("shared:critic:<name>" against
"<case>:critic:<name>").  Stored per case: the parameter names (the critic's state_dict names), state_drones, cylinders and value [B, A, 1].
"""
import os

import numpy as np
import torch
import torch.nn as nn

import make_golden_policy as MP

# (tag, rows, drones, cylinders, state_drones width, seed)
CASES = [("a3k3d35", 6, 3, 3, 35, 201), ("a1k3d20", 6, 1, 3, 20, 202), ("a4k5d20", 5, 4, 5, 20, 203)]


def main():
    torch.set_num_threads(1)
    _, PAE, _, _, Critic = MP.load()
    out, shared = {}, None
    for tag, B, A, K, D, seed in CASES:
        torch.manual_seed(seed)
        spec = MP._Composite()
        spec["state_drones"] = MP._Spec(B, A, D)
        spec["cylinders"] = MP._Spec(B, K, 5)
        v_out = nn.Linear(128, A)
        nn.init.orthogonal_(v_out.weight, 0.01)
        critic = Critic(PAE(spec), None, v_out, torch.Size((A, 1)))
        g = torch.Generator().manual_seed(seed + 1000)
        MP.perturb(critic, g)
        if shared is None:
            shared = {n: p.detach().clone() for n, p in critic.state_dict().items()}
        else:
            with torch.no_grad():
                for n, p in critic.state_dict().items():
                    if shared[n].shape == p.shape:
                        p.copy_(shared[n])
        state = {"state_drones": torch.randn(B, A, D, generator=g) * 0.7}
        cyl = torch.randn(B, K, 5, generator=g) * 0.5
        cyl[:, K // 2:, :] = torch.where(torch.rand(B, K - K // 2, 1, generator=g) < 0.4, torch.zeros(()), cyl[:, K // 2:, :])
        state["cylinders"] = cyl                    # some inactive slots of zeros, kept in the attention as the env writes them
        with torch.no_grad():
            value, _ = critic(state)
        assert tuple(value.shape) == (B, A, 1)
        out[f"{tag}:shape"] = np.array([B, A, K, D])
        names = []
        for n, p in critic.state_dict().items():
            names.append(n)
            if tag != CASES[0][0] and torch.equal(shared[n], p):
                continue
            out[f"{tag}:critic:{n}"] = MP.bf16_bits(p)
        out[f"{tag}:critic_names"] = np.array(names)
        out[f"{tag}:state_drones"], out[f"{tag}:cylinders"], out[f"{tag}:value"] = state["state_drones"].numpy(), cyl.numpy(), value.numpy()
    first = CASES[0][0]
    for n in list(shared):
        out[f"shared:critic:{n}"] = out.pop(f"{first}:critic:{n}")
    path = os.path.join(MP.M.OUT, "g_policy_central.npz")
    np.savez_compressed(path, cases=np.array([c[0] for c in CASES]), **out)
    print(f"g_policy_central: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
