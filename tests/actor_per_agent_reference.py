"""Test-side restatement of MAPPOPolicy.update_actor with share_actor: False (learning/mappo.py:271-324, the else branch at :288-291) in any
float dtype: a loop over the agents' slices of the STACKED actor on tests/actor_update_reference.py's statements — agent a's rows through slice
a's log-probability, then the same surrogate, entropy mean, ESS and autograd over the stacked tensors.  fp64 autograd is the accuracy gate's
yardstick, fp32 the CPU error it is measured against.  `stacked_actor` builds genuinely different agents from one shared actor (the recipe of
g_actor_per_agent.npz); `sample_actions` / `new_log_probs` are the per-agent forms of the shared file's helpers."""
import math

import numpy as np
import torch

import actor_update_reference as U

ACT_DIM = U.ACT_DIM


def stacked_actor(actor, A, seed):
    """{name: float32 [A, ...]}: `actor` ({name: array}, one shared actor) perturbed per agent and tensor by a seeded generator — 0.05 sigma,
    log_std 0.2 sigma and a further 0.1 a, so that no two agents share a tensor or a scale."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in U._strip(actor).items():
        v = torch.as_tensor(np.asarray(v), dtype=torch.float32)
        sig = 0.2 if k.endswith("log_std") else 0.05
        rows = [v + torch.randn(v.shape, generator=g) * sig + (0.1 * a if k.endswith("log_std") else 0.0) for a in range(A)]
        out[k] = torch.stack(rows).contiguous().numpy()
    return out


def agent(actors, a):
    return {k: np.asarray(v)[a] for k, v in actors.items()}


def _obs_of(obs, a):
    return {k: v[:, a:a + 1] for k, v in obs.items()}


def loss_and_grad(actors, obs, action, log_probs_old, advantages, index=None, clip_param=0.1, entropy_coef=0.001, dtype=torch.float64):
    """actors: {reference name: array [A, ...]}; the other arguments and the returned dict as actor_update_reference.loss_and_grad, with
    grads {name: float64 numpy [A, ...]} of policy_loss - entropy_coef entropy over ALL B A rows and entropy the mean over the agents."""
    p, o, act, lpo, adv = U._prep(actors, obs, action, log_probs_old, advantages, index, dtype)
    names = list(p)
    A = act.shape[1]
    n = float(adv.numel())
    logp = torch.cat([U.log_prob({k: v[a] for k, v in p.items()}, _obs_of(o, a), act[:, a:a + 1], dtype) for a in range(A)], dim=1)
    assert logp.shape == lpo.shape == adv.shape
    ratio = torch.exp(logp - lpo)
    surr = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param) * adv)
    ent = (0.5 + 0.5 * math.log(2 * math.pi) + p["act_dist.log_std"]).sum(-1).reshape(1, A, 1).expand(logp.shape)     # per agent, on every row
    total = -(surr * ACT_DIM).sum() / n + entropy_coef * (-(ent.sum() / n))
    grads = torch.autograd.grad(total, [p[k] for k in names])
    with torch.no_grad():
        ess = (2 * ratio.logsumexp(0) - (2 * ratio).logsumexp(0)).exp().mean() / ratio.shape[0]
        norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads))
        w = U.clip_weight(ratio, adv, clip_param)
    return {"policy_loss": float(-(surr.detach() * ACT_DIM).mean()), "entropy": float(ent.detach().mean()), "ess": float(ess), "grad_norm": float(norm),
            "log_probs": logp.detach().double().numpy(), "ratio": ratio.detach().double().numpy(), "adv": adv.double().numpy(), "w": w.double().numpy(),
            "grads": {k: g.detach().double().numpy() for k, g in zip(names, grads)}}


def new_log_probs(actors, obs, action, dtype=torch.float64):
    """The agents' log-probabilities of `action` [S, A, 4]: [S, A, 1] numpy in `dtype`."""
    A = obs["state_self"].shape[1]
    act = np.asarray(action).reshape(-1, A, ACT_DIM)
    return np.concatenate([U.new_log_probs(agent(actors, a), _obs_of(obs, a), act[:, a:a + 1], dtype) for a in range(A)], axis=1)


def sample_actions(actors, obs, seed, sigmas=1.0):
    """mu_a + sigma_a eps per agent from an fp32 forward pass: [S, A, 4] float32."""
    A = obs["state_self"].shape[1]
    return np.concatenate([U.sample_actions(agent(actors, a), _obs_of(obs, a), seed + a, sigmas) for a in range(A)], axis=1)


def golden_case(za, zp, tag):
    """One case of g_actor_per_agent.npz (tests/golden/make_golden_actor_per_agent.py): (stacked actor {name: fp32 [A, ...]} in the module's
    parameter order — rebuilt by `stacked_actor` from g_policy.npz's actor, as the generator built it — obs, action, log_probs_old,
    advantages, index, entropy_coef, recorded {key: array})."""
    import policy_reference as R
    base, _, _, _, _ = R.golden_case(zp, str(za[f"{tag}:base"]))
    obs = {k: za[f"{tag}:obs:{k}"] for k in ("state_self", "state_others", "cylinders") if f"{tag}:obs:{k}" in za.files}
    A = obs["state_self"].shape[1]
    actors = stacked_actor({str(n): base[str(n)] for n in za[f"{tag}:names"]}, A, int(za[f"{tag}:param_seed"]))
    rec = {k[len(tag) + 1:]: za[k] for k in za.files if k.startswith(tag + ":")}
    return actors, obs, za[f"{tag}:action"], za[f"{tag}:log_probs_old"], za[f"{tag}:advantages"], za[f"{tag}:index"], float(za[f"{tag}:entropy_coef"]), rec
