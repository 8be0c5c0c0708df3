"""What the tests of recurrent per-agent actors share (test_per_agent_rnn.py on the CPU, test_hip_per_agent_rnn.py on the device; share_actor:
False with actor.rnn / critic.rnn): the parameter sets and the fp64 / fp32 references, in numpy under the reference's names.

The stacked actor holds an encoder, a GRU and a head per agent (every tensor [A, ...]); the critic and the critic's GRU are shared.  Its
references are tests/policy_rnn_reference.py's run PER SLICE: agent a's rows of `RR.forward(slice a, critic, ...)` on the whole observation.

  golden_params  the networks of g_policy_rnn_per_agent.npz (tests/golden/make_golden_policy_rnn_per_agent.py): policy_rnn_reference.golden_params
                 of the base case — g_policy.npz's encoder and head, g_gru.npz's GRU, the critic's GRU its ih / hh exchange — with the ACTOR
                 (its GRU included) perturbed per agent and tensor by actor_per_agent_reference.stacked_actor
  random_net     policy_rnn_reference.random_net per agent (independent seeds), stacked"""
import hashlib

import numpy as np
import torch

import actor_per_agent_reference as UA
import policy_reference as R
import policy_rnn_reference as RR

# (tag, g_policy case of the base networks, envs, pursuers, cylinders, state_self width, steps, the steps with flags, seed)
GOLDEN_CASES = [("a3k5d35", "a3k5d35", 11, 3, 5, 35, 5, (0, 3), 501), ("a2k8d20", "a3k8d20", 4, 2, 8, 20, 3, (0,), 502)]
CASES = tuple(c[0] for c in GOLDEN_CASES)
GOLDEN_TOL = 1e-5                                            # what test_policy_rnn.py applies to g_policy_rnn.npz
OUTPUTS = RR.OUTPUTS


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(np.asarray(t, np.float32)).tobytes())
    return h.hexdigest()


def golden_params(gp, gg, base_tag, A, seed):
    """(stacked actor {name: fp32 [A, ...]}, critic {name: fp32}) of a golden case, rebuilt from g_policy.npz and g_gru.npz."""
    actor, critic = RR.golden_params(gp, gg, base_tag)
    return UA.stacked_actor(actor, A, seed), critic


def golden_case(z, gp, gg, tag):
    """(stacked actor, critic, {name: array} of the case) of g_policy_rnn_per_agent.npz; the rebuilt tensors are held to the file's digest."""
    case = RR.golden_case(z, tag)
    E, A = (int(v) for v in case["shape"][:2])
    actors, critic = golden_params(gp, gg, str(case["base"]), A, int(case["param_seed"]))
    assert digest([actors[k] for k in sorted(actors)] + [critic[k] for k in sorted(critic)]) == str(case["init_digest"]), tag
    return actors, critic, case


def agent(actors, a):
    return {k: np.asarray(v)[a] for k, v in actors.items()}


def random_net(D, A, seed):
    """(stacked actor, critic): A independently drawn recurrent actors (policy_rnn_reference.random_net at seeds seed + 1000 a; no two agents
    share a tensor, a scale or a LayerNorm affine), the critic the first draw's."""
    nets = [RR.random_net(D, A, seed + 1000 * a) for a in range(A)]
    return {k: np.stack([n[0][k] for n in nets]) for k in nets[0][0]}, nets[0][1]


def random_flags(E, seed, p=0.4):
    """Mixed env-level flags [E] bool: env 0 set, the last env clear (E = 1: set)."""
    f = np.random.default_rng(seed).random(E) < p
    f[0] = True
    if E > 1:
        f[-1] = False
    return f


def slice_forward(actors, critic, obs, actor_state, critic_state, is_init, eps, dtype):
    """{name: numpy in `dtype`} of one step: agent a's rows from policy_rnn_reference.forward with slice a as the shared actor, on the whole
    observation and state; value and the critic's state from the first call (they do not depend on the actor)."""
    A = np.asarray(obs["state_self"]).shape[1]
    outs = [RR.forward(agent(actors, a), critic, obs, actor_state, critic_state, is_init, eps, dtype) for a in range(A)]
    out = {k: torch.cat([o[k][:, a:a + 1] for a, o in enumerate(outs)], dim=1) for k in ("loc", "log_prob", "action", "actor_state")}
    out["value"], out["critic_state"] = outs[0]["value"], outs[0]["critic_state"]
    return {k: v.numpy() for k, v in out.items()}


def chain_references(actors, critic, obs, eps, flags, ha, hc):
    """[(fp64 outputs, fp32 outputs)] per step of a chain, each dtype's chain feeding itself (policy_rnn_cases.chain_references per slice)."""
    h = {torch.float64: (ha, hc), torch.float32: (ha, hc)}
    out = []
    for t in range(len(obs)):
        step = []
        for dtype in (torch.float64, torch.float32):
            r = slice_forward(actors, critic, obs[t], *h[dtype], flags[t], eps[t], dtype)
            h[dtype] = (r["actor_state"], r["critic_state"])
            step.append({k: np.asarray(v, np.float64) for k, v in r.items()})
        out.append(tuple(step))
    return out
