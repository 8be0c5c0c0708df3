#!/usr/bin/env python3
"""Generate tests/golden/g_policy_rnn.npz by EXECUTING the reference's recurrent policy networks (authoring container only: needs the reference
checkout; never run on the GPU box, never from tests).  Reuses make_golden_policy.load() and make_golden.load_by_path without changing them.

The reference's own Actor(PartialAttentionEncoder, DiagGaussian, GRU(128, 128)) and Critic(PartialAttentionEncoder, GRU(128, 128), v_out, (1,))
(learning/mappo.py:591-660, modules/rnn.py:32-89), as make_ppo_actor / make_critic build them with cfg.rnn set, on CPU fp32 with one thread.
No parameter is stored here: the encoder and head parameters are g_policy.npz's of the case of the same tag, the GRUs' are g_gru.npz's
(tests/policy_rnn_reference.py::golden_params assembles them, for this script and for the tests alike).

MAPPOPolicy calls the networks through vmap over the agent dimension with the env-level is_init expanded to every agent (mappo.py:221-250), so
each agent's call sees [E, ...] rows, a state [E, 128] and flags [E, 1]: here a loop over the agents makes those calls.  Per step Actor.forward
runs twice on the same inputs: deterministic (the mode = loc, and the new state), then eval_action on action = loc + scale eps (the
reparameterised sample with the standard-normal draw made explicit, as g_policy.npz has it) for the distribution's own log_prob.
Cases (tag, envs, pursuers, cylinders, state_self width, steps, the steps whose is_init is set for some envs):
  a3k5d35  E 11, A 3, K 5, D 35, 5 chained one-step calls, flags at steps 0 and 3
  a1k5d20  E 4,  A 1, K 5, D 20, 3 steps, flags at step 0
The states start from 0.5 N(0, 1) (so a flag at step 0 matters) and are chained through the reference's own outputs.
Stored per case: obs:<key> [T, E, A, ..], eps [T, E, A, 4], is_init [T, E], h0:actor, h0:critic [E, A, 128], and per step loc, action, log_prob,
value, actor_state, critic_state (the states AFTER the step)."""
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
import policy_rnn_reference as RR  # noqa: E402

RNN = "omni_drones/learning/modules/rnn.py"
CASES = [("a3k5d35", 11, 3, 5, 35, 5, (0, 3), 201), ("a1k5d20", 4, 1, 5, 20, 3, (0,), 202)]


def main():
    torch.set_num_threads(1)
    _, PAE, DiagGaussian, Actor, Critic = MP.load()
    GRU = M.load_by_path("ref_rnn", RNN).GRU
    gp, gg = np.load(os.path.join(M.OUT, "g_policy.npz")), np.load(os.path.join(M.OUT, "g_gru.npz"))
    out = {}
    for tag, E, A, K, D, T, flag_steps, seed in CASES:
        torch.manual_seed(seed)
        spec = MP._Composite()
        spec["state_self"] = MP._Spec(E, A, 1, D)
        if A > 1:
            spec["state_others"] = MP._Spec(E, A, A - 1, 3)
        spec["cylinders"] = MP._Spec(E, A, K, 5)
        actor = Actor(PAE(spec), DiagGaussian(128, 4, False, 0.01), GRU(128, 128))
        critic = Critic(PAE(spec), GRU(128, 128), nn.Linear(128, 1), torch.Size((1,)))
        pa, pc = RR.golden_params(gp, gg, tag)
        actor.load_state_dict({k: torch.as_tensor(v) for k, v in pa.items()}, strict=True)
        critic.load_state_dict({k: torch.as_tensor(v) for k, v in pc.items()}, strict=True)
        g = torch.Generator().manual_seed(seed + 1000)
        ha, hc = 0.5 * torch.randn(E, A, 128, generator=g), 0.5 * torch.randn(E, A, 128, generator=g)
        out[f"{tag}:shape"] = np.array([E, A, K, D, T])
        out[f"{tag}:h0:actor"], out[f"{tag}:h0:critic"] = ha.numpy().copy(), hc.numpy().copy()
        rec = {k: [] for k in ("obs:state_self", "obs:state_others", "obs:cylinders", "eps", "is_init", "loc", "action", "log_prob", "value",
                               "actor_state", "critic_state")}
        for t in range(T):
            obs = {"state_self": torch.randn(E, A, 1, D, generator=g) * 0.7}
            if A > 1:
                obs["state_others"] = torch.randn(E, A, A - 1, 3, generator=g) * 0.5
            obs["cylinders"] = torch.randn(E, A, K, 5, generator=g) * 0.5
            eps = torch.randn(E, A, 4, generator=g)
            flags = torch.zeros(E, 1, dtype=torch.bool)
            if t in flag_steps:
                flags = torch.rand(E, 1, generator=g) < 0.4
                flags[0], flags[1] = True, False
            step = {k: [] for k in ("loc", "action", "log_prob", "value", "actor_state", "critic_state")}
            with torch.no_grad():
                for a in range(A):                       # vmap over the agents: each call sees [E, ...]
                    o = {k: v[:, a] for k, v in obs.items()}
                    loc, _, _, h_new = actor(o, rnn_state=ha[:, a], is_init=flags, deterministic=True)
                    scale = actor.act_dist(torch.zeros(1, 128)).base_dist.scale[0]
                    action = loc + scale * eps[:, a]
                    _, logp, _, _ = actor(o, action=action, rnn_state=ha[:, a], is_init=flags, eval_action=True)
                    value, c_new = critic(o, hc[:, a], flags)
                    for k, v in (("loc", loc), ("action", action), ("log_prob", logp), ("value", value), ("actor_state", h_new), ("critic_state", c_new)):
                        step[k].append(v)
            step = {k: torch.stack(v, 1) for k, v in step.items()}
            assert step["log_prob"].shape == (E, A, 1) and step["value"].shape == (E, A, 1) and step["actor_state"].shape == (E, A, 128)
            ha, hc = step["actor_state"], step["critic_state"]
            for k, v in obs.items():
                rec["obs:" + k].append(v.numpy())
            rec["eps"].append(eps.numpy())
            rec["is_init"].append(flags[:, 0].numpy())
            for k, v in step.items():
                rec[k].append(v.numpy())
        for k, v in rec.items():
            if v:
                out[f"{tag}:{k}"] = np.stack(v)
        assert out[f"{tag}:is_init"][0].any() and not out[f"{tag}:is_init"].all()
    path = os.path.join(M.OUT, "g_policy_rnn.npz")
    np.savez_compressed(path, cases=np.array([c[0] for c in CASES]), **out)
    print(f"g_policy_rnn: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
