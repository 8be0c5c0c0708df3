#!/usr/bin/env python3
"""Generate tests/golden/g_actor_per_agent.npz by EXECUTING the reference's actor update with cfg.share_actor = False (authoring container only:
needs the reference checkout; never run on the GPU box, never from tests).  Built as make_golden_actor_update.py is, whose loaders and helpers
it reuses unchanged.

The reference's own Actor + DiagGaussian + PartialAttentionEncoder run the statements of MAPPOPolicy.update_actor (mappo.py:271-324) as written,
on CPU fp32 with one thread.  With share_actor: False the reference holds ONE module (actors[0]) and the STACKED parameters of A of them
(mappo.py:148-152) and calls `vmap(self.actor, in_dims=(1, 0), out_dims=1)` (mappo.py:288-291); torchrl / tensordict are not installed, so the
exec namespace gets a stand-in `vmap` that does what that call does, one agent at a time: dim 1 of the input and dim 0 of the stacked
parameters are indexed, the reference's module runs functionally on agent a's slice (torch.func.functional_call), the outputs are stacked on
dim 1.  ONE torch.optim.Adam(lr 5e-4) and one clip_grad_norm_(max_grad_norm 10) over the stacked tensors — the reference's actor_opt — twice in a
row on the same minibatch.

The agents are genuinely different: g_policy.npz's actor perturbed per agent and tensor (tests/actor_per_agent_reference.stacked_actor; the
tests rebuild the same tensors, `init_digest` pins them).  Cases, 24 env-steps each and a shuffled index of 17, log_probs_old off the clip
by make_golden_actor_update.py's recipe:
  a3k5d35  (g_policy's a3k5d35 actor)            entropy_coef 0.001
  a2k8d20  (g_policy's a3k8d20 actor, 2 agents)  entropy_coef 0.001, advantages times 40: the clip of the norm is active
Stored per case what g_actor_update.npz stores: obs, action, log_probs_old, advantages, index, entropy_coef; per update policy_loss, entropy,
ESS, grad_norm and a sha256 over all clipped gradients; the clipped gradients of update 1 and the parameters after the two updates for the
small tensors ([A, ...]), the 128-wide ones pinned by the digests."""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as M  # noqa: E402
import make_golden_policy as MP  # noqa: E402
import make_golden_actor_update as GU  # noqa: E402

sys.path.insert(0, os.path.dirname(M.OUT))
import policy_reference as R  # noqa: E402
import actor_per_agent_reference as UA  # noqa: E402

# (tag, g_policy case of the base actor, pursuers, cylinders, state_self width, seed, entropy_coef, advantage scale)
CASES = [("a3k5d35", "a3k5d35", 3, 5, 35, 401, 0.001, 0.2), ("a2k8d20", "a3k8d20", 2, 8, 20, 402, 0.001, 0.2 * 40)]
S, B = GU.S, GU.B
LOGP, ENT = GU.LOGP, GU.ENT


def main():
    torch.set_num_threads(1)
    _, PAE, DiagGaussian, Actor, _ = MP.load()
    stmts = M._stmt_sources(GU.MAPPO, "MAPPOPolicy", "update_actor", lambda s: not s.startswith("return"))
    assert any("vmap(self.actor, in_dims=(1, 0), out_dims=1)" in s for s in stmts) and any("clip_grad_norm_" in s for s in stmts), stmts
    gp = np.load(os.path.join(M.OUT, "g_policy.npz"))
    out = {}
    for tag, base_tag, A, K, D, seed, ent_coef, adv_scale in CASES:
        base, _, _, _, _ = R.golden_case(gp, base_tag)
        spec = MP._Composite()
        spec["state_self"] = MP._Spec(S, A, 1, D)
        spec["state_others"] = MP._Spec(S, A, A - 1, 3)
        spec["cylinders"] = MP._Spec(S, A, K, 5)
        actor = Actor(PAE(spec), DiagGaussian(128, 4, False, 0.01), None)
        names = [n for n, _ in actor.named_parameters()]
        init = UA.stacked_actor({n: base[n] for n in names}, A, seed + 50)
        stacked = {n: torch.nn.Parameter(torch.as_tensor(init[n])) for n in names}
        g = torch.Generator().manual_seed(seed)
        obs = {"state_self": torch.randn(S, A, 1, D, generator=g) * 0.7, "state_others": torch.randn(S, A, A - 1, 3, generator=g) * 0.5,
               "cylinders": torch.randn(S, A, K, 5, generator=g) * 0.5}

        def one(actor_input, params, eval_action):                # self.actor on one agent's input and parameters
            _, lp, ent, _ = torch.func.functional_call(actor, params, (actor_input["obs"],), {"action": actor_input["action"], "eval_action": eval_action})
            return {LOGP: lp, ENT: ent}

        def vmap(fn, in_dims, out_dims):
            assert in_dims == (1, 0) and out_dims == 1

            def mapped(actor_input, params, **kw):
                outs = [fn({"obs": {k: t[:, a] for k, t in actor_input["obs"].items()}, "action": actor_input["action"][:, a]},
                           {n: t[a] for n, t in params.items()}, **kw) for a in range(A)]
                return {k: torch.stack([o[k] for o in outs], dim=1) for k in outs[0]}
            return mapped

        with torch.no_grad():
            lp0 = vmap(one, (1, 0), 1)({"obs": obs, "action": torch.zeros(S, A, 4)}, stacked, eval_action=True)          # (for the shapes only)
            locs = []
            for a in range(A):
                d = torch.func.functional_call(actor.act_dist, {k[len("act_dist."):]: v[a] for k, v in stacked.items() if k.startswith("act_dist.")},
                                               (torch.func.functional_call(actor.encoder, {k[len("encoder."):]: v[a] for k, v in stacked.items()
                                                                                           if k.startswith("encoder.")}, ({k: t[:, a] for k, t in obs.items()},)),))
                locs.append((d.base_dist.loc, d.base_dist.scale))
            action = torch.stack([l + s * torch.randn(S, 4, generator=g) for l, s in locs], dim=1).contiguous()
            logp = vmap(one, (1, 0), 1)({"obs": obs, "action": action}, stacked, eval_action=True)[LOGP]
        assert logp.shape == lp0[LOGP].shape == (S, A, 1)
        band = torch.rand(logp.shape, generator=g) < 0.5
        mag = torch.where(band, 0.05 * torch.rand(logp.shape, generator=g), 0.15 + 0.25 * torch.rand(logp.shape, generator=g))
        delta = mag * torch.where(torch.rand(logp.shape, generator=g) < 0.5, -1.0, 1.0)
        logp_old = (logp - delta).contiguous()
        adv = (torch.randn(logp.shape, generator=g) * adv_scale).contiguous()
        index = torch.randperm(S, generator=g)[:B]
        ratio0 = torch.exp(logp - logp_old)[index].double()
        assert float(torch.minimum((ratio0 - 0.9).abs(), (ratio0 - 1.1).abs()).min()) > 0.03, tag
        batch = GU._Batch({"obs": {k: t[index] for k, t in obs.items()}, "action": action[index], LOGP: logp_old[index], "advantages": adv[index]})
        batch.batch_size = (B,)
        opt = torch.optim.Adam(list(stacked.values()), lr=5e-4)
        self = types.SimpleNamespace(actor_in_keys=["obs", "action"], act_logps_name=LOGP, agent_spec=types.SimpleNamespace(n=A, name="drone"),
                                     clip_param=0.1, act_dim=4, actor=one, actor_params=stacked, actor_opt=opt,
                                     cfg=types.SimpleNamespace(share_actor=False, max_grad_norm=10.0, entropy_coef=ent_coef,
                                                               actor=types.SimpleNamespace(tanh=False)))
        for k, t in obs.items():
            out[f"{tag}:obs:{k}"] = t.numpy()
        out[f"{tag}:action"], out[f"{tag}:log_probs_old"], out[f"{tag}:advantages"] = action.numpy(), logp_old.numpy(), adv.numpy()
        out[f"{tag}:index"], out[f"{tag}:entropy_coef"], out[f"{tag}:names"] = index.numpy(), np.float64(ent_coef), np.array(names)
        out[f"{tag}:base"], out[f"{tag}:param_seed"] = np.array(base_tag), np.int64(seed + 50)
        out[f"{tag}:init_digest"] = np.array(GU.digest([stacked[n] for n in names]))
        for u in (1, 2):
            ns = {"self": self, "batch": batch, "torch": torch, "vmap": vmap}
            for code in stmts:
                exec(code, ns)
                if "actor_opt.step()" in code:                   # after clip_grad_norm_ and the step: the clipped gradients
                    grads = {n: p.grad.clone() for n, p in stacked.items()}
            for k, t in (("policy_loss", ns["policy_loss"]), ("entropy", -ns["entropy_loss"]), ("ESS", ns["ess"]), ("grad_norm", ns["grad_norm"])):
                out[f"{tag}:u{u}:{k}"] = t.detach().numpy().copy()
            out[f"{tag}:u{u}:grad_digest"] = np.array(GU.digest([grads[n] for n in names]))
            if u == 1:
                print(f"{tag}: policy_loss {float(ns['policy_loss'].detach()):.6f} entropy {float(-ns['entropy_loss'].detach()):.6f} ESS {float(ns['ess'].detach()):.6f} "
                      f"norm {float(ns['grad_norm']):.3f}")
                for n in names:
                    if n not in GU.BIG:
                        out[f"{tag}:grad:{n}"] = grads[n].numpy()
        out[f"{tag}:final_digest"] = np.array(GU.digest([stacked[n] for n in names]))
        for n in names:
            if n not in GU.BIG:
                out[f"{tag}:final:{n}"] = stacked[n].detach().numpy().copy()
    assert float(out["a2k8d20:u1:grad_norm"]) > 10.0 and float(out["a3k5d35:u1:grad_norm"]) < 10.0
    path = os.path.join(M.OUT, "g_actor_per_agent.npz")
    np.savez_compressed(path, cases=np.array([c[0] for c in CASES]), **out)
    print(f"g_actor_per_agent: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
