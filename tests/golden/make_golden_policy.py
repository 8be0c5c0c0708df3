#!/usr/bin/env python3
"""Generate tests/golden/g_policy.npz by EXECUTING the reference's policy networks (authoring container only: needs the reference checkout;
never run on the GPU box, never from tests).  Reuses make_golden.py's loaders without changing that file.

The reference's own SplitEmbedding and PartialAttentionEncoder (learning/modules/networks.py:125-163, :250-313), DiagGaussian
(modules/distributions.py:66-82), Actor and Critic (learning/mappo.py:591-660) run on CPU in fp32, built as make_ppo_actor / make_critic build
them for HideAndSeek's CompositeSpec observation (cfg/algo/mappo.yaml: attn_encoder PartialAttentionEncoder, gain 0.01, v_out orthogonal).
Each case starts from the constructors' initialisation under a fixed seed; the biases, the LayerNorm affine parameters and log_std are then
perturbed so that no term is trivially 0 or 1, and every parameter is rounded to 8 significant bits (bfloat16 values).
To keep the file small, every later case takes the first case's parameters wherever the shapes agree (so only the state_self embedding's weight,
whose width is the case's D, is its own), and the parameters are stored once, as their bfloat16 bits (uint16):
"shared:<actor|critic>:<name>" for the first case's, "<case>:<actor|critic>:<name>" for a case's own.  The action is Actor.forward's `action_dist.sample()` with the standard-normal draw made
explicit (loc + scale eps, the reparameterised sample), its log_prob the distribution's own; the mode is `action_dist.mode`.
Stored per case: the parameter names (state_dict names of the actor and the critic), the observations, eps, loc, action, log_prob,
value and mode.
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as M  # noqa: E402

NETWORKS = "omni_drones/learning/modules/networks.py"
DISTRIBUTIONS = "omni_drones/learning/modules/distributions.py"
MAPPO = "omni_drones/learning/mappo.py"
# (tag, envs, pursuers, cylinders, state_self width, seed)
CASES = [("a3k5d35", 16, 3, 5, 35, 101), ("a3k8d20", 16, 3, 8, 20, 102), ("a1k5d20", 16, 1, 5, 20, 103), ("a6k16d24", 8, 6, 16, 24, 104)]


class _Spec:
    def __init__(self, *shape):
        self.shape = torch.Size(shape)


class _Composite(dict):
    pass


def _classes(relpath, names, ns):
    src = open(os.path.join(M.REF, relpath)).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.ClassDef) and node.name in names:
            exec(compile(ast.get_source_segment(src, node), f"<ref:{node.name}>", "exec"), ns)
    return [ns[n] for n in names]


def load():
    from typing import Optional, Union
    ns = {"D": torch.distributions, "torch": torch, "nn": nn, "F": F, "Tensor": torch.Tensor, "Optional": Optional, "Union": Union, "CompositeSpec": _Composite,
          "TensorDict": dict}
    SplitEmbedding, PAE = _classes(NETWORKS, ["SplitEmbedding", "PartialAttentionEncoder"], ns)
    M.exec_functions(M.extract_source(DISTRIBUTIONS, ["init"]), ns)
    (DiagGaussian,) = _classes(DISTRIBUTIONS, ["DiagGaussian"], ns)
    Actor, Critic = _classes(MAPPO, ["Actor", "Critic"], ns)
    return SplitEmbedding, PAE, DiagGaussian, Actor, Critic


def perturb(module, g):
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("bias") or "norm" in name or name.endswith("log_std"):
                p.add_(torch.randn(p.shape, generator=g) * (0.3 if "log_std" in name else 0.1))
            p.copy_(p.to(torch.bfloat16).float())      # 8 significant bits: the file stays small, the network runs on these values


def main():
    torch.set_num_threads(1)
    _, PAE, DiagGaussian, Actor, Critic = load()
    out = {}
    shared = {}                                     # which -> {name: tensor} of the first case (parameters of the same shape in every case)
    for tag, E, A, K, D, seed in CASES:
        torch.manual_seed(seed)
        spec = _Composite()
        spec["state_self"] = _Spec(E, A, 1, D)
        if A > 1:
            spec["state_others"] = _Spec(E, A, A - 1, 3)
        spec["cylinders"] = _Spec(E, A, K, 5)
        actor = Actor(PAE(spec), DiagGaussian(128, 4, False, 0.01), None)
        v_out = nn.Linear(128, 1)
        nn.init.orthogonal_(v_out.weight, 0.01)
        critic = Critic(PAE(spec), None, v_out, torch.Size((1,)))
        g = torch.Generator().manual_seed(seed + 1000)
        perturb(actor, g)
        perturb(critic, g)
        for which, net in (("actor", actor), ("critic", critic)):
            if which not in shared:
                shared[which] = {n: p.detach().clone() for n, p in net.state_dict().items()}
                continue
            with torch.no_grad():                   # later cases take every parameter whose shape matches the first case's
                for n, p in net.state_dict().items():
                    if n in shared[which] and shared[which][n].shape == p.shape:
                        p.copy_(shared[which][n])
        obs = {"state_self": torch.randn(E, A, 1, D, generator=g) * 0.7}
        if A > 1:
            obs["state_others"] = torch.randn(E, A, A - 1, 3, generator=g) * 0.5
        cyl = torch.randn(E, A, K, 5, generator=g) * 0.5
        cyl[:, :, K // 2:, :] = torch.where(torch.rand(E, 1, K - K // 2, 1, generator=g) < 0.4, torch.zeros(()), cyl[:, :, K // 2:, :])
        obs["cylinders"] = cyl                      # some inactive slots of zeros, kept in the attention as the env writes them
        eps = torch.randn(E, A, 4, generator=g)
        with torch.no_grad():
            d = actor.act_dist(actor.encoder(obs))
            loc, scale = d.base_dist.loc, d.base_dist.scale
            action = loc + scale * eps
            logp = d.log_prob(action).unsqueeze(-1)
            mode = d.mode
            value, _ = critic(obs)
        out[f"{tag}:shape"] = np.array([E, A, K, D])
        for which, net in (("actor", actor), ("critic", critic)):
            names = []
            for n, p in net.state_dict().items():
                names.append(n)
                if tag != CASES[0][0] and n in shared[which] and torch.equal(shared[which][n], p):
                    continue                        # stored once, under shared:<which>:<name>
                out[f"{tag}:{which}:{n}"] = bf16_bits(p)
            out[f"{tag}:{which}_names"] = np.array(names)
        for k, v in obs.items():
            out[f"{tag}:obs:{k}"] = v.numpy()
        for k, v in (("eps", eps), ("loc", loc), ("action", action), ("log_prob", logp), ("value", value), ("mode", mode)):
            out[f"{tag}:{k}"] = v.numpy()
    first = CASES[0][0]
    for which in ("actor", "critic"):                # the first case's parameters are the shared ones
        for n in list(shared[which]):
            out[f"shared:{which}:{n}"] = out.pop(f"{first}:{which}:{n}")
    path = os.path.join(M.OUT, "g_policy.npz")
    np.savez_compressed(path, cases=np.array([c[0] for c in CASES]), **out)
    print(f"g_policy: {os.path.getsize(path) / 1024:.1f} KB")


def bf16_bits(p):
    """The parameter's bfloat16 value as its 16 bits (uint16): exact, since perturb() rounded every parameter to bfloat16."""
    b = p.detach().contiguous().view(torch.int32).numpy().astype(np.uint32)
    assert np.all(b & 0xFFFF == 0)
    return (b >> 16).astype(np.uint16)


if __name__ == "__main__":
    main()
