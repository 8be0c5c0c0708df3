#!/usr/bin/env python3
"""Generate tests/golden/g_policy_rnn_per_agent.npz by EXECUTING the reference's recurrent policy networks with the STACKED actor of
cfg.share_actor = False (authoring container only: needs the reference checkout; never run on the GPU box, never from tests).  Built as
make_golden_policy_rnn.py and make_golden_actor_per_agent.py are, whose loaders it reuses unchanged.

The reference's own Actor(PartialAttentionEncoder, DiagGaussian, GRU(128, 128)) and Critic(PartialAttentionEncoder, GRU(128, 128), v_out, (1,))
(learning/mappo.py:591-660, modules/rnn.py:32-89) on CPU fp32 with one thread.  With share_actor: False the reference holds ONE actor module and
the STACKED parameters of A of them — the actor's GRU among them — (mappo.py:148-152) and calls
`vmap(self.actor, in_dims=(1, 0), out_dims=1, randomness="different")` (mappo.py:243-246); torchrl / tensordict are not installed, so a stand-in
does what that call does, one agent at a time: dim 1 of the input (observation, state) and dim 0 of the stacked parameters are indexed, the
reference's module runs functionally on agent a's slice (torch.func.functional_call), the outputs are stacked on dim 1.  The critic is one
module, vmapped over the agent axis with its own parameters (mappo.py:247-250): a loop over the agents.  Per step the actor runs twice on the same
inputs, as make_golden_policy_rnn.py has it: deterministic (loc and the new state), then eval_action on action = loc + scale eps.

No parameter is stored: tests/per_agent_rnn_cases.golden_params rebuilds them (g_policy.npz's encoder and head and g_gru.npz's GRU, the actor
perturbed per agent and tensor by actor_per_agent_reference.stacked_actor), for this script and for the tests alike; `init_digest` pins them.
Cases (tag, base case of g_policy.npz, envs, pursuers, cylinders, state_self width, steps, the steps whose is_init is set for some envs):
  a3k5d35  a3k5d35, E 11, A 3, K 5, D 35, 5 chained one-step calls, flags at steps 0 and 3
  a2k8d20  a3k8d20, E 4,  A 2, K 8, D 20, 3 steps, flags at step 0
The states start from 0.5 N(0, 1) and are chained through the reference's own outputs.
Asserted here: for every pair a != b and every step, agent a's loc computed with agent b's slice differs from its own by at least 100 times the
tolerance the test applies (a swapped or repeated image cannot pass).
Stored per case: shape, base, param_seed, init_digest, obs:<key> [T, E, A, ..], eps [T, E, A, 4], is_init [T, E], h0:actor, h0:critic
[E, A, 128], and per step loc, action, log_prob, value, actor_state, critic_state (the states AFTER the step)."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as M  # noqa: E402
import make_golden_policy as MP  # noqa: E402
import per_agent_rnn_cases as C  # noqa: E402

RNN = "omni_drones/learning/modules/rnn.py"


def main():
    torch.set_num_threads(1)
    _, PAE, DiagGaussian, Actor, Critic = MP.load()
    GRU = M.load_by_path("ref_rnn", RNN).GRU
    gp, gg = np.load(os.path.join(M.OUT, "g_policy.npz")), np.load(os.path.join(M.OUT, "g_gru.npz"))
    out = {}
    for tag, base, E, A, K, D, T, flag_steps, seed in C.GOLDEN_CASES:
        torch.manual_seed(seed)
        spec = MP._Composite()
        spec["state_self"] = MP._Spec(E, A, 1, D)
        spec["state_others"] = MP._Spec(E, A, A - 1, 3)
        spec["cylinders"] = MP._Spec(E, A, K, 5)
        actor = Actor(PAE(spec), DiagGaussian(128, 4, False, 0.01), GRU(128, 128))
        critic = Critic(PAE(spec), GRU(128, 128), nn.Linear(128, 1), torch.Size((1,)))
        pa, pc = C.golden_params(gp, gg, base, A, seed + 50)
        assert set(pa) == {n for n, _ in actor.named_parameters()}, sorted(set(pa) ^ {n for n, _ in actor.named_parameters()})
        stacked = {n: torch.as_tensor(v) for n, v in pa.items()}
        critic.load_state_dict({k: torch.as_tensor(v) for k, v in pc.items()}, strict=True)

        def vmap(fn, in_dims, out_dims):
            assert in_dims == (1, 0) and out_dims == 1

            def mapped(actor_input, params, **kw):
                outs = [fn({k: (t[:, a] if torch.is_tensor(t) else {n: v[:, a] for n, v in t.items()}) for k, t in actor_input.items()},
                           {n: t[a] for n, t in params.items()}, **kw) for a in range(A)]
                return tuple(torch.stack([o[i] for o in outs], dim=1) if outs[0][i] is not None else None for i in range(len(outs[0])))
            return mapped

        def one(actor_input, params, is_init, **kw):          # self.actor on one agent's input and parameters
            return torch.func.functional_call(actor, params, (actor_input["obs"],),
                                              {"rnn_state": actor_input["state"], "is_init": is_init, "action": actor_input.get("action"), **kw})

        g = torch.Generator().manual_seed(seed + 1000)
        ha, hc = 0.5 * torch.randn(E, A, 128, generator=g), 0.5 * torch.randn(E, A, 128, generator=g)
        out[f"{tag}:shape"] = np.array([E, A, K, D, T])
        out[f"{tag}:base"], out[f"{tag}:param_seed"] = np.array(base), np.int64(seed + 50)
        out[f"{tag}:init_digest"] = np.array(C.digest([pa[k] for k in sorted(pa)] + [pc[k] for k in sorted(pc)]))
        out[f"{tag}:h0:actor"], out[f"{tag}:h0:critic"] = ha.numpy().copy(), hc.numpy().copy()
        rec = {k: [] for k in ("obs:state_self", "obs:state_others", "obs:cylinders", "eps", "is_init", "loc", "action", "log_prob", "value",
                               "actor_state", "critic_state")}
        gap = float("inf")
        for t in range(T):
            obs = {"state_self": torch.randn(E, A, 1, D, generator=g) * 0.7, "state_others": torch.randn(E, A, A - 1, 3, generator=g) * 0.5,
                   "cylinders": torch.randn(E, A, K, 5, generator=g) * 0.5}
            eps = torch.randn(E, A, 4, generator=g)
            flags = torch.zeros(E, 1, dtype=torch.bool)
            if t in flag_steps:
                flags = torch.rand(E, 1, generator=g) < 0.4
                flags[0], flags[1] = True, False
            with torch.no_grad():
                loc, _, _, h_new = vmap(one, (1, 0), 1)({"obs": obs, "state": ha}, stacked, is_init=flags, deterministic=True)
                scale = torch.exp(stacked["act_dist.log_std"]).unsqueeze(0)              # DiagGaussian: scale = exp(log_std), per agent
                action = (loc + scale * eps).contiguous()
                _, logp, _, _ = vmap(one, (1, 0), 1)({"obs": obs, "state": ha, "action": action}, stacked, is_init=flags, eval_action=True)
                vc = [critic({k: v[:, a] for k, v in obs.items()}, hc[:, a], flags) for a in range(A)]
                value, c_new = torch.stack([v for v, _ in vc], 1), torch.stack([h for _, h in vc], 1)
                for a in range(A):                                # agent a's rows through every OTHER agent's slice
                    for b in range(A):
                        if a != b:
                            other = one({"obs": {k: v[:, a] for k, v in obs.items()}, "state": ha[:, a]}, {n: v[b] for n, v in stacked.items()},
                                        flags, deterministic=True)[0]
                            gap = min(gap, float((other - loc[:, a]).abs().max()))
            step = {"loc": loc, "action": action, "log_prob": logp, "value": value, "actor_state": h_new, "critic_state": c_new}
            assert logp.shape == (E, A, 1) and value.shape == (E, A, 1) and h_new.shape == c_new.shape == (E, A, 128)
            ha, hc = h_new, c_new
            for k, v in obs.items():
                rec["obs:" + k].append(v.numpy())
            rec["eps"].append(eps.numpy())
            rec["is_init"].append(flags[:, 0].numpy())
            for k, v in step.items():
                rec[k].append(v.numpy())
        for k, v in rec.items():
            out[f"{tag}:{k}"] = np.stack(v)
        assert out[f"{tag}:is_init"][0].any() and not out[f"{tag}:is_init"].all()
        assert gap >= 100 * C.GOLDEN_TOL, (tag, gap)
        print(f"{tag}: the smallest loc difference under another agent's slice {gap:.3e} (>= {100 * C.GOLDEN_TOL:.0e})")
    path = os.path.join(M.OUT, "g_policy_rnn_per_agent.npz")
    np.savez_compressed(path, cases=np.array(C.CASES), **out)
    print(f"g_policy_rnn_per_agent: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
