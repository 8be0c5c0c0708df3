#!/usr/bin/env python3
"""Generate tests/golden/g_critic_update.npz by EXECUTING the reference's critic update (authoring container only: needs the reference
checkout; never run on the GPU box, never from tests).  Reuses make_golden.py's and make_golden_policy.py's loaders without changing them.

The reference's own Critic + PartialAttentionEncoder (learning/mappo.py:630-660, modules/networks.py:250-313), built as make_critic builds them
for HideAndSeek's observation (v_out orthogonal, gain 0.01), run the statements of MAPPOPolicy.update_critic (mappo.py:326-352) as written, one
statement at a time, on CPU fp32 with one thread: nn.HuberLoss(delta=10) or nn.MSELoss(), clip_param 0.1, clip_grad_norm_ at max_grad_norm 10,
torch.optim.Adam(lr 5e-4, weight_decay 0), twice in a row on the same minibatch.  `self.value_op` is the critic called on the minibatch's
observation (the reference vmaps the same module over the agent dimension, which this network treats as a batch dimension anyway).

Cases: the four shapes of g_policy.npz with THAT file's critic parameters (bfloat16 values; nothing is stored twice), 24 env-steps of fresh
observations and an index that is a shuffled strict subset of 17 of them.  Old values / returns per case:
  a3k5d35  Huber, half of the rows with old values 0.3 nearer to the returns than the new ones: the unclipped mean is the larger (branch 0)
  a3k8d20  Huber, half of the rows 0.3 further: the clipped mean is the larger (branch 1)
  a1k5d20  Huber, returns times 40: rows leave the delta, the total norm exceeds max_grad_norm (the clip is active); half 0.5 nearer (branch 0)
  a6k16d24 MSE, half 0.3 further (branch 1)
Stored per case: obs, b_values, b_returns, index; per update u = 1, 2: value_loss, l_orig, l_clip, grad_norm (clip_grad_norm_'s return value),
explained_var; the branch of update 1; the clipped gradients of update 1 — all of them for the first case, the vectors / embeddings / head and
linear2.weight for the others; a sha256 over all clipped gradients of each update and over all parameters after the two updates; the parameters
after the two updates — the vectors, the small embeddings and the head (and linear2.weight for the first case); the other matrices are pinned
by the digest.
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as M  # noqa: E402
import make_golden_policy as MP  # noqa: E402

sys.path.insert(0, os.path.dirname(M.OUT))
import policy_reference as R  # noqa: E402

MAPPO = "omni_drones/learning/mappo.py"
# (tag, pursuers, cylinders, state_self width, seed, loss, shift, returns scale)
CASES = [("a3k5d35", 3, 5, 35, 201, "huber", +0.3, 1.0), ("a3k8d20", 3, 8, 20, 202, "huber", -0.3, 1.0),
         ("a1k5d20", 1, 5, 20, 203, "huber", +0.5, 40.0), ("a6k16d24", 6, 16, 24, 204, "mse", -0.3, 1.0)]
S, B = 24, 17
BIG = ("base.attn.in_proj_weight", "base.attn.out_proj.weight", "base.linear1.weight", "base.linear2.weight", "base.split_embed.embed.state_self.weight")


class _Batch(dict):
    def select(self, *keys):
        return _Batch({k: self[k] for k in keys})


def digest(tensors):
    return hashlib.sha256(b"".join(np.ascontiguousarray(t.detach().numpy(), dtype=np.float32).tobytes() for t in tensors)).hexdigest()


def main():
    torch.set_num_threads(1)
    _, PAE, _, _, Critic = MP.load()
    stmts = M._stmt_sources(MAPPO, "MAPPOPolicy", "update_critic", lambda s: not s.startswith("return"))
    assert any("torch.max(value_loss_original, value_loss_clipped)" in s for s in stmts) and any("clip_grad_norm_" in s for s in stmts), stmts
    gp = np.load(os.path.join(M.OUT, "g_policy.npz"))
    out = {}
    for tag, A, K, D, seed, loss, shift, ret_scale in CASES:
        _, params, _, _, _ = R.golden_case(gp, tag)
        spec = MP._Composite()
        spec["state_self"] = MP._Spec(S, A, 1, D)
        if A > 1:
            spec["state_others"] = MP._Spec(S, A, A - 1, 3)
        spec["cylinders"] = MP._Spec(S, A, K, 5)
        critic = Critic(PAE(spec), None, nn.Linear(128, 1), torch.Size((1,)))
        critic.load_state_dict({k: torch.as_tensor(v) for k, v in params.items()})
        names = [n for n, _ in critic.named_parameters()]
        g = torch.Generator().manual_seed(seed)
        obs = {"state_self": torch.randn(S, A, 1, D, generator=g) * 0.7}
        if A > 1:
            obs["state_others"] = torch.randn(S, A, A - 1, 3, generator=g) * 0.5
        obs["cylinders"] = torch.randn(S, A, K, 5, generator=g) * 0.5
        with torch.no_grad():
            v = critic(obs)[0]
        ret = ((v + torch.randn(v.shape, generator=g)) * ret_scale).contiguous()
        bv = v + torch.randn(v.shape, generator=g) * 0.03
        if shift is not None:
            half = torch.rand(v.shape, generator=g) < 0.5
            bv = torch.where(half, v + shift * torch.sign(ret - v), bv)
        index = torch.randperm(S, generator=g)[:B]
        batch = _Batch({"obs": {k: t[index] for k, t in obs.items()}, "state_value": bv[index], "returns": ret[index]})
        self = types.SimpleNamespace(critic_in_keys=["obs"], clip_param=0.1, critic=critic, cfg=types.SimpleNamespace(max_grad_norm=10.0),
                                     critic_loss_fn=nn.HuberLoss(delta=10) if loss == "huber" else nn.MSELoss(),
                                     critic_opt=torch.optim.Adam(critic.parameters(), lr=5e-4, weight_decay=0.0))
        self.value_op = lambda ci: {"state_value": critic(ci["obs"])[0]}
        for k, t in obs.items():
            out[f"{tag}:obs:{k}"] = t.numpy()
        out[f"{tag}:b_values"], out[f"{tag}:b_returns"], out[f"{tag}:index"] = bv.numpy(), ret.numpy(), index.numpy()
        out[f"{tag}:loss"] = np.array(loss)
        out[f"{tag}:names"] = np.array(names)
        for u in (1, 2):
            ns = {"self": self, "batch": batch, "torch": torch, "nn": nn, "F": F}
            for code in stmts:
                exec(code, ns)
                if "critic_opt.step()" in code:                  # after clip_grad_norm_ and the step, before zero_grad: the clipped gradients
                    grads = {n: p.grad.clone() for n, p in critic.named_parameters()}
            lo, lc = ns["value_loss_original"], ns["value_loss_clipped"]
            for k, t in (("value_loss", ns["value_loss"]), ("l_orig", lo), ("l_clip", lc), ("grad_norm", ns["grad_norm"]), ("explained_var", ns["explained_var"])):
                out[f"{tag}:u{u}:{k}"] = t.detach().numpy().copy()
            out[f"{tag}:u{u}:grad_digest"] = np.array(digest([grads[n] for n in names]))
            if u == 1:
                lo, lc = lo.detach(), lc.detach()
                branch = 0 if float(lo) > float(lc) else (1 if float(lo) < float(lc) else 2)
                assert abs(float(lo) - float(lc)) >= 2e-3 * float(ns["value_loss"]), tag      # no case on the tie of the max
                out[f"{tag}:branch"] = np.int64(branch)
                print(f"{tag}: l_orig {float(lo):.6f} l_clip {float(lc):.6f} branch {branch} norm {float(ns['grad_norm']):.3f}")
                for n in names:
                    if tag == CASES[0][0] or n not in BIG or n == "base.linear2.weight":
                        out[f"{tag}:grad:{n}"] = grads[n].numpy()
        final = dict(critic.named_parameters())
        out[f"{tag}:final_digest"] = np.array(digest([final[n] for n in names]))
        for n in names:
            if n not in BIG or (tag == CASES[0][0] and n == "base.linear2.weight"):
                out[f"{tag}:final:{n}"] = final[n].detach().numpy().copy()
    b = {t[0]: int(out[f"{t[0]}:branch"]) for t in CASES}
    assert b == {"a3k5d35": 0, "a3k8d20": 1, "a1k5d20": 0, "a6k16d24": 1}, b
    assert float(out["a1k5d20:u1:grad_norm"]) > 10.0
    path = os.path.join(M.OUT, "g_critic_update.npz")
    np.savez_compressed(path, cases=np.array([c[0] for c in CASES]), **out)
    print(f"g_critic_update: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
