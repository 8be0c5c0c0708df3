"""Test-side restatement of MAPPOPolicy.update_actor (learning/mappo.py:271-324) in any float dtype, on top of tests/policy_reference.py (the
full attention over all tokens, written out from the equations, independent of hns_amd): the DiagGaussian log-probability, the clipped PPO
surrogate, the entropy bonus, ESS, and the gradients by torch autograd.  fp64 autograd is the accuracy gate's yardstick, fp32 the CPU error it is
measured against.  `hand_grads` is the per-row rule the kernel implements (d logp = -k adv r w / n, w from the clip), pushed through autograd
of logp alone: it must agree with autograd of the loss.  `make_old_log_probs` builds data that stays off the clip's discontinuity."""
import math

import numpy as np
import torch

import policy_reference as R

ACT_DIM = 4


def _strip(d):
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in d.items()}


def _prep(actor, obs, action, log_probs_old, advantages, index, dtype):
    p = {k: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in _strip(actor).items()}
    idx = torch.as_tensor(np.asarray(index)) if index is not None else None
    take = lambda v: torch.as_tensor(np.asarray(v))[idx] if idx is not None else torch.as_tensor(np.asarray(v))
    o = {k: take(v) for k, v in obs.items()}
    S = o["state_self"].shape[0]
    A = o["state_self"].shape[1]
    act = take(np.asarray(action).reshape(-1, A, ACT_DIM)).to(dtype)
    lpo = take(np.asarray(log_probs_old).reshape(-1, A, 1)).to(dtype)
    adv = take(np.asarray(advantages).reshape(-1, A, 1)).to(dtype)
    assert act.shape[0] == lpo.shape[0] == adv.shape[0] == S
    return p, o, act, lpo, adv


def log_prob(p, o, act, dtype):
    """Normal(mu, exp(log_std)).log_prob(action) summed over the action dimension: [.., 1]."""
    mu = R._lin(R.encoder(p, "encoder.", o, dtype), p["act_dist.fc_mean.weight"], p["act_dist.fc_mean.bias"])
    ls = p["act_dist.log_std"]
    sigma = torch.exp(ls)
    return (-((act - mu) ** 2) / (2 * sigma ** 2) - torch.log(sigma) - math.log(math.sqrt(2 * math.pi))).sum(-1, keepdim=True)


def clip_weight(ratio, adv, clip_param):
    """The backward weight of torch.min(surr1, surr2) and clamp together: 1 inside the clip (bounds included), outside 1 where the unclipped
    surrogate is the smaller, else 0."""
    inside = (ratio >= 1.0 - clip_param) & (ratio <= 1.0 + clip_param)
    s1, s2 = ratio * adv, ratio.clamp(1.0 - clip_param, 1.0 + clip_param) * adv
    return torch.where(inside, torch.ones_like(ratio), (s1 < s2).to(ratio.dtype))


def loss_and_grad(actor, obs, action, log_probs_old, advantages, index=None, clip_param=0.1, entropy_coef=0.001, dtype=torch.float64, chunk=8192,
                  hand=False):
    """actor: {reference name: array}; obs over S env-steps; action [S, A, 4]; log_probs_old, advantages [S, A, 1]; index: env-steps of the
    minibatch.  Returns a dict: policy_loss, entropy, ess, grad_norm (floats), log_probs, ratio, adv, w (float64 numpy [B, A, 1]) and grads
    {name: float64 numpy} of policy_loss - entropy_coef entropy.  The loss is a sum over rows, so a minibatch of more than `chunk` env-steps runs
    chunk by chunk (the attention over all tokens in fp64 does not fit in memory) and the gradients add up.  hand=True: the gradients by the
    per-row rule instead of autograd of the loss."""
    p, o, act, lpo, adv = _prep(actor, obs, action, log_probs_old, advantages, index, dtype)
    names = list(p)
    B = act.shape[0]
    n = float(adv.numel())
    grads, loss_sum, logps = None, 0.0, []
    for s in range(0, B, chunk):
        e = min(s + chunk, B)
        logp = log_prob(p, {k: v[s:e] for k, v in o.items()}, act[s:e], dtype)
        assert logp.shape == lpo[s:e].shape == adv[s:e].shape
        ratio = torch.exp(logp - lpo[s:e])
        surr = torch.min(ratio * adv[s:e], torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param) * adv[s:e])
        ent = (0.5 + 0.5 * math.log(2 * math.pi) + p["act_dist.log_std"]).sum().expand(logp.shape)
        if hand:
            w = clip_weight(ratio.detach(), adv[s:e], clip_param)
            dlogp = -ACT_DIM * adv[s:e] * ratio.detach() * w / n
            gs = list(torch.autograd.grad(logp, [p[k] for k in names], grad_outputs=dlogp))
            if s == 0:
                k = names.index("act_dist.log_std")
                gs[k] = gs[k] - entropy_coef
        else:
            part = -(surr * ACT_DIM).sum() / n + entropy_coef * (-(ent.sum() / n))
            gs = torch.autograd.grad(part, [p[k] for k in names])
        grads = gs if grads is None else [a + b for a, b in zip(grads, gs)]
        loss_sum = loss_sum + float(-(surr.detach().double() * ACT_DIM).sum())
        logps.append(logp.detach())
    with torch.no_grad():
        logp = torch.cat(logps)
        ratio = torch.exp(logp - lpo)
        ess = (2 * ratio.logsumexp(0) - (2 * ratio).logsumexp(0)).exp().mean() / ratio.shape[0]
        entropy = float((0.5 + 0.5 * math.log(2 * math.pi) + p["act_dist.log_std"]).sum())
        norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads))
        w = clip_weight(ratio, adv, clip_param)
        surr = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param) * adv)
        policy_loss = float(-(surr * ACT_DIM).mean()) if B <= chunk else loss_sum / n
    return {"policy_loss": policy_loss, "entropy": entropy, "ess": float(ess), "grad_norm": float(norm), "log_probs": logp.double().numpy(),
            "ratio": ratio.double().numpy(), "adv": adv.double().numpy(), "w": w.double().numpy(),
            "grads": {k: g.detach().double().numpy() for k, g in zip(names, grads)}}


def new_log_probs(actor, obs, action, dtype=torch.float64, chunk=4096):
    """The actor's log-probabilities of `action` [S, A, 4] over all S env-steps: [S, A, 1] numpy in `dtype`."""
    p = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in _strip(actor).items()}
    A = obs["state_self"].shape[1]
    act = torch.as_tensor(np.asarray(action).reshape(-1, A, ACT_DIM)).to(dtype)
    out = []
    with torch.no_grad():
        for s in range(0, act.shape[0], chunk):
            out.append(log_prob(p, {k: torch.as_tensor(v[s:s + chunk]) for k, v in obs.items()}, act[s:s + chunk], dtype).numpy())
    return np.concatenate(out)


def sample_actions(actor, obs, seed, sigmas=1.0, chunk=4096):
    """mu + sigma eps (eps standard normal times `sigmas`) from an fp32 forward pass: [S, A, 4] float32."""
    p = {k: torch.as_tensor(np.asarray(v)) for k, v in _strip(actor).items()}
    g = np.random.default_rng(seed)
    out = []
    with torch.no_grad():
        for s in range(0, obs["state_self"].shape[0], chunk):
            o = {k: torch.as_tensor(v[s:s + chunk]) for k, v in obs.items()}
            mu = R._lin(R.encoder(p, "encoder.", o, torch.float32), p["act_dist.fc_mean.weight"], p["act_dist.fc_mean.bias"]).numpy()
            out.append(mu + np.exp(np.asarray(p["act_dist.log_std"])) * g.standard_normal(mu.shape) * sigmas)
    return np.concatenate(out).astype(np.float32)


def make_old_log_probs(logp_new, seed, bands=((0.0, 0.05), (0.15, 0.40))):
    """log_probs_old = logp_new - delta with |delta| in [0, 0.05] or [0.15, 0.40], both signs: every ratio exp(delta) is >= 0.039 away from
    1 +- 0.1 (log 1.1 = 0.0953 and -log 0.9 = 0.1054 lie in the excluded band).  Returns float32 [.., 1]."""
    g = np.random.default_rng(seed)
    pick = g.integers(0, len(bands), logp_new.shape)
    lo = np.array([b[0] for b in bands])[pick]
    hi = np.array([b[1] for b in bands])[pick]
    delta = (lo + (hi - lo) * g.random(logp_new.shape)) * np.where(g.random(logp_new.shape) < 0.5, -1.0, 1.0)
    return (np.asarray(logp_new, np.float64) - delta).astype(np.float32)


def assert_off_the_clip(r64, clip_param=0.1, margin=1e-3, need_all=True):
    """In fp64: no ratio within `margin` of 1 +- clip_param; rows with w = 0, rows with w = 1 outside the clip and rows inside it all occur."""
    ratio, w = r64["ratio"], r64["w"]
    dist = np.minimum(np.abs(ratio - (1 - clip_param)), np.abs(ratio - (1 + clip_param)))
    assert dist.min() >= margin, f"a ratio is {dist.min():.2e} from the clip's bound"
    inside = (ratio >= 1 - clip_param) & (ratio <= 1 + clip_param)
    if need_all:
        assert (w == 0).any() and ((w == 1) & ~inside).any() and inside.any(), ((w == 0).sum(), ((w == 1) & ~inside).sum(), inside.sum())
    return float(dist.min())


def golden_case(za, zp, tag):
    """One case of g_actor_update.npz (tests/golden/make_golden_actor_update.py) with its actor parameters from g_policy.npz: (actor {name:
    fp32 array} in the module's parameter order, obs, action, log_probs_old, advantages, index, entropy_coef, recorded {key: array})."""
    actor, _, _, _, _ = R.golden_case(zp, tag)
    actor = {str(n): actor[str(n)] for n in za[f"{tag}:names"]}
    obs = {k: za[f"{tag}:obs:{k}"] for k in ("state_self", "state_others", "cylinders") if f"{tag}:obs:{k}" in za.files}
    rec = {k[len(tag) + 1:]: za[k] for k in za.files if k.startswith(tag + ":")}
    return actor, obs, za[f"{tag}:action"], za[f"{tag}:log_probs_old"], za[f"{tag}:advantages"], za[f"{tag}:index"], float(za[f"{tag}:entropy_coef"]), rec
