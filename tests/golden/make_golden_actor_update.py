#!/usr/bin/env python3
"""Generate tests/golden/g_actor_update.npz by EXECUTING the reference's actor update (authoring container only: needs the reference
checkout; never run on the GPU box, never from tests).  Reuses make_golden.py's and make_golden_policy.py's loaders without changing them.

The reference's own Actor + DiagGaussian + PartialAttentionEncoder (learning/mappo.py:591-628, modules/distributions.py:66-82,
modules/networks.py:250-313), built as make_ppo_actor builds them for HideAndSeek's observation, run the statements of
MAPPOPolicy.update_actor (mappo.py:271-324) as written, one statement at a time, on CPU fp32 with one thread: clip_param 0.1, act_dim 4,
clip_grad_norm_ at max_grad_norm 10, torch.optim.Adam(lr 5e-4), twice in a row on the same minibatch.  `self.actor` is the module called on
the minibatch's observation and stored action with eval_action=True (the reference wraps the same module in a TensorDictModule).

Cases: the four shapes of g_policy.npz with THAT file's actor parameters (bfloat16 values; nothing is stored twice), 24 env-steps of fresh
observations, actions mu + sigma eps, and an index that is a shuffled strict subset of 17 of the env-steps.  log_probs_old = logp_new - delta
with |delta| in [0, 0.05] or [0.15, 0.40], both signs (every ratio of update 1 is >= 0.039 away from 1 +- 0.1), advantages 0.2 x standard normal (both signs).
  a3k5d35  entropy_coef 0.001
  a3k8d20  entropy_coef 0.001, advantages times 40: the total norm exceeds max_grad_norm (the clip of the norm is active)
  a1k5d20  entropy_coef 0
  a6k16d24 entropy_coef 0.001
Stored per case: obs, action, log_probs_old, advantages, index, entropy_coef; per update u = 1, 2: policy_loss, entropy, ESS, grad_norm
(clip_grad_norm_'s return value) and a sha256 over all clipped gradients; the clipped gradients of update 1 and the parameters after the two
updates — the vectors, the small embeddings, the head and log_std in full; the 128-wide matrices are pinned by the digests.
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as M  # noqa: E402
import make_golden_policy as MP  # noqa: E402

sys.path.insert(0, os.path.dirname(M.OUT))
import policy_reference as R  # noqa: E402

MAPPO = "omni_drones/learning/mappo.py"
# (tag, pursuers, cylinders, state_self width, seed, entropy_coef, advantage scale)
CASES = [("a3k5d35", 3, 5, 35, 301, 0.001, 0.2), ("a3k8d20", 3, 8, 20, 302, 0.001, 0.2 * 40), ("a1k5d20", 1, 5, 20, 303, 0.0, 0.2),
         ("a6k16d24", 6, 16, 24, 304, 0.001, 0.2)]
S, B = 24, 17
BIG = ("encoder.attn.in_proj_weight", "encoder.attn.out_proj.weight", "encoder.linear1.weight", "encoder.linear2.weight",
       "encoder.split_embed.embed.state_self.weight")
LOGP, ENT = "drone.action_logp", "drone.action_entropy"


class _Batch(dict):
    batch_size = ()

    def select(self, *keys):
        out = _Batch({k: self[k] for k in keys})
        out.batch_size = self.batch_size
        return out


def digest(tensors):
    return hashlib.sha256(b"".join(np.ascontiguousarray(t.detach().numpy(), dtype=np.float32).tobytes() for t in tensors)).hexdigest()


def main():
    torch.set_num_threads(1)
    _, PAE, DiagGaussian, Actor, _ = MP.load()
    stmts = M._stmt_sources(MAPPO, "MAPPOPolicy", "update_actor", lambda s: not s.startswith("return"))
    assert any("torch.min(surr1, surr2)" in s for s in stmts) and any("clip_grad_norm_" in s for s in stmts) and any("logsumexp" in s for s in stmts), stmts
    gp = np.load(os.path.join(M.OUT, "g_policy.npz"))
    out = {}
    for tag, A, K, D, seed, ent_coef, adv_scale in CASES:
        params, _, _, _, _ = R.golden_case(gp, tag)
        spec = MP._Composite()
        spec["state_self"] = MP._Spec(S, A, 1, D)
        if A > 1:
            spec["state_others"] = MP._Spec(S, A, A - 1, 3)
        spec["cylinders"] = MP._Spec(S, A, K, 5)
        actor = Actor(PAE(spec), DiagGaussian(128, 4, False, 0.01), None)
        actor.load_state_dict({k: torch.as_tensor(v) for k, v in params.items()})
        names = [n for n, _ in actor.named_parameters()]
        g = torch.Generator().manual_seed(seed)
        obs = {"state_self": torch.randn(S, A, 1, D, generator=g) * 0.7}
        if A > 1:
            obs["state_others"] = torch.randn(S, A, A - 1, 3, generator=g) * 0.5
        obs["cylinders"] = torch.randn(S, A, K, 5, generator=g) * 0.5
        with torch.no_grad():
            d = actor.act_dist(actor.encoder(obs))
            action = (d.base_dist.loc + d.base_dist.scale * torch.randn(S, A, 4, generator=g)).contiguous()
            logp = d.log_prob(action).unsqueeze(-1)
        band = torch.rand(logp.shape, generator=g) < 0.5
        mag = torch.where(band, 0.05 * torch.rand(logp.shape, generator=g), 0.15 + 0.25 * torch.rand(logp.shape, generator=g))
        delta = mag * torch.where(torch.rand(logp.shape, generator=g) < 0.5, -1.0, 1.0)
        logp_old = (logp - delta).contiguous()
        adv = (torch.randn(logp.shape, generator=g) * adv_scale).contiguous()
        index = torch.randperm(S, generator=g)[:B]
        ratio0 = torch.exp(logp - logp_old)[index].double()
        assert float(torch.minimum((ratio0 - 0.9).abs(), (ratio0 - 1.1).abs()).min()) > 0.03, tag
        batch = _Batch({"obs": {k: t[index] for k, t in obs.items()}, "action": action[index], LOGP: logp_old[index], "advantages": adv[index]})
        batch.batch_size = (B,)
        opt = torch.optim.Adam(actor.parameters(), lr=5e-4)

        def call(actor_input, actor_params, eval_action):
            _, lp, ent, _ = actor(actor_input["obs"], action=actor_input["action"], eval_action=eval_action)
            return {LOGP: lp, ENT: ent}

        self = types.SimpleNamespace(actor_in_keys=["obs", "action"], act_logps_name=LOGP, agent_spec=types.SimpleNamespace(n=A, name="drone"),
                                     clip_param=0.1, act_dim=4, actor=call, actor_params=None, actor_opt=opt,
                                     cfg=types.SimpleNamespace(share_actor=True, max_grad_norm=10.0, entropy_coef=ent_coef,
                                                               actor=types.SimpleNamespace(tanh=False)))
        for k, t in obs.items():
            out[f"{tag}:obs:{k}"] = t.numpy()
        out[f"{tag}:action"], out[f"{tag}:log_probs_old"], out[f"{tag}:advantages"] = action.numpy(), logp_old.numpy(), adv.numpy()
        out[f"{tag}:index"], out[f"{tag}:entropy_coef"], out[f"{tag}:names"] = index.numpy(), np.float64(ent_coef), np.array(names)
        for u in (1, 2):
            ns = {"self": self, "batch": batch, "torch": torch}
            for code in stmts:
                exec(code, ns)
                if "actor_opt.step()" in code:                   # after clip_grad_norm_ and the step: the clipped gradients
                    grads = {n: p.grad.clone() for n, p in actor.named_parameters()}
            for k, t in (("policy_loss", ns["policy_loss"]), ("entropy", -ns["entropy_loss"]), ("ESS", ns["ess"]), ("grad_norm", ns["grad_norm"])):
                out[f"{tag}:u{u}:{k}"] = t.detach().numpy().copy()
            out[f"{tag}:u{u}:grad_digest"] = np.array(digest([grads[n] for n in names]))
            if u == 1:
                print(f"{tag}: policy_loss {float(ns['policy_loss'].detach()):.6f} entropy {float(-ns['entropy_loss'].detach()):.6f} ESS {float(ns['ess'].detach()):.6f} "
                      f"norm {float(ns['grad_norm']):.3f}")
                for n in names:
                    if n not in BIG:
                        out[f"{tag}:grad:{n}"] = grads[n].numpy()
        final = dict(actor.named_parameters())
        out[f"{tag}:final_digest"] = np.array(digest([final[n] for n in names]))
        for n in names:
            if n not in BIG:
                out[f"{tag}:final:{n}"] = final[n].detach().numpy().copy()
    assert float(out["a3k8d20:u1:grad_norm"]) > 10.0 and all(float(out[f"{t}:u1:grad_norm"]) < 10.0 for t in ("a3k5d35", "a1k5d20", "a6k16d24"))
    path = os.path.join(M.OUT, "g_actor_update.npz")
    np.savez_compressed(path, cases=np.array([c[0] for c in CASES]), **out)
    print(f"g_actor_update: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
