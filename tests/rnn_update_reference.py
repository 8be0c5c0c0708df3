"""Test-side reference of the recurrent MAPPO update (hns_amd.rnn_train) in any float dtype, independent of hns_amd.rnn_train:

  * `actor_head_autograd` / `critic_head_autograd`: torch.autograd of the reference's statements (update_actor / update_critic, mappo.py:271-352:
    torch.distributions, torch.min / clamp, nn.HuberLoss, torch.max of two means) on given rows y [B, L, A, 128], with the [B, L, A, 1] ESS;
  * `flow`: a whole update up to backward() — policy_reference.encoder, an nn.GRUCell stepped in a Python loop with the carried state multiplied
    by 1 - is_init, LayerNorm(h + x), a torch head, the same loss statements, .backward();
  * `head_case`: the head entries' inputs (log_probs_old off the clip as tests/actor_update_reference.py builds it, b_values off the value clip,
    returns that choose the branch of the max);
  * `predictor` / `predictor_rollout`: a TPNet and its rollout entries (tests/learner_cases.py's shapes, TP_done all ones) for the learner tests;
  * `gate`: the project's rule, e <= BAR max(e_32, 2^-24 max|ref_64|), BAR = 8, per tensor and scalar."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import actor_update_reference as UA
import policy_reference as R

H = 128
BAR = 8.0
MARGIN = 1e-3


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x)).to(dtype)


def actor_statements(y, w, b, log_std, action, lpo, adv, clip_param, entropy_coef):
    """update_actor's statements (mappo.py:293-318 behind DiagGaussian.forward) on y [B, L, A, 128]; action [B, L, A, 4], lpo / adv [B, L, A, 1]."""
    mean = F.linear(y, w, b)
    dist = torch.distributions.Independent(torch.distributions.Normal(mean, torch.exp(log_std).expand_as(mean), validate_args=False), 1, validate_args=False)
    log_probs = dist.log_prob(action).unsqueeze(-1)
    dist_entropy = dist.entropy().unsqueeze(-1)
    ratio = torch.exp(log_probs - lpo)
    surr1 = ratio * adv
    surr2 = torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param) * adv
    policy_loss = -torch.mean(torch.min(surr1, surr2) * 4)
    entropy_loss = -torch.mean(dist_entropy)
    with torch.no_grad():
        ess = (2 * ratio.logsumexp(0) - (2 * ratio).logsumexp(0)).exp().mean() / ratio.shape[0]
        inside = (ratio >= 1.0 - clip_param) & (ratio <= 1.0 + clip_param)
        wgt = (inside | (surr1 < surr2)).double()
    scal = {"policy_loss": policy_loss.detach(), "entropy": -entropy_loss.detach(), "ess": ess, "log_probs": log_probs.detach().squeeze(-1),
            "ratio": ratio.detach().squeeze(-1), "w": wgt.squeeze(-1)}
    return policy_loss + entropy_loss * entropy_coef, scal


def critic_statements(y, w, b, bv, ret, clip_param, loss, huber_delta):
    """update_critic's statements (mappo.py:328-341) on y [B, L, A, 128]; bv / ret [B, L, A, 1]."""
    values = F.linear(y, w, b)
    clipped = bv + (values - bv).clamp(-clip_param, clip_param)
    loss_fn = nn.HuberLoss(delta=huber_delta) if loss == "huber" else nn.MSELoss()
    l_clip, l_orig = loss_fn(ret, clipped), loss_fn(ret, values)
    value_loss = torch.max(l_orig, l_clip)
    with torch.no_grad():
        explained_var = 1 - F.mse_loss(values, ret) / ret.var()
    scal = {"value_loss": value_loss.detach(), "explained_var": explained_var, "values": values.detach().squeeze(-1), "l_orig": l_orig.detach(),
            "l_clip": l_clip.detach(), "dist": ((values - bv).abs() - clip_param).abs().min().detach()}
    return value_loss, scal


def _np(d):
    return {k: (v.detach().double().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}


def actor_head_autograd(case, dtype, clip_param=0.1, entropy_coef=1e-3):
    """{dy, d_head_w, d_head_b, d_log_std, policy_loss, entropy, ess, log_probs, ratio, w} as fp64 numpy."""
    y, w, b, ls = (_t(case[k], dtype).requires_grad_(True) for k in ("y", "head_w", "head_b", "log_std"))
    total, scal = actor_statements(y, w, b, ls, _t(case["action"], dtype), _t(case["log_probs_old"], dtype).unsqueeze(-1),
                                   _t(case["advantages"], dtype).unsqueeze(-1), clip_param, entropy_coef)
    g = torch.autograd.grad(total, [y, w, b, ls])
    return _np({"dy": g[0], "d_head_w": g[1], "d_head_b": g[2], "d_log_std": g[3], **scal})


def critic_head_autograd(case, dtype, clip_param=0.1, loss="huber", huber_delta=10.0):
    y, w, b = (_t(case[k], dtype).requires_grad_(True) for k in ("y", "v_w", "v_b"))
    total, scal = critic_statements(y, w, b, _t(case["b_values"], dtype).unsqueeze(-1), _t(case["b_returns"], dtype).unsqueeze(-1), clip_param, loss,
                                    huber_delta)
    g = torch.autograd.grad(total, [y, w, b])
    return _np({"dy": g[0], "d_head_w": g[1], "d_head_b": g[2], **scal})


def assert_off_the_edges(a64, c64, clip_param=0.1, tie=False):
    """In fp64: no ratio within 1e-3 of 1 +- clip_param, no |v - b_values| within 1e-3 of clip_param; off the tie of the max unless `tie`."""
    ratio = a64["ratio"]
    d = np.minimum(np.abs(ratio - (1 - clip_param)), np.abs(ratio - (1 + clip_param)))
    assert d.min() >= MARGIN, f"a ratio is {d.min():.2e} from the clip's bound"
    assert float(c64["dist"]) >= MARGIN, f"a value is {float(c64['dist']):.2e} from the value clip's bound"
    sep = abs(float(c64["l_orig"]) - float(c64["l_clip"]))
    if tie:
        assert sep == 0.0, f"the two mean losses differ by {sep:.3e}: not the tie"
    else:
        assert sep >= 1e-3 * float(c64["value_loss"]), f"the two mean losses are {sep:.3e} apart: too near the tie of the max"


def head_case(B, L, A, seed, bands=((0.0, 0.05), (0.15, 0.40)), branch="orig", head_scale=0.1, value_bands=((0.0, 0.05), (0.15, 0.40))):
    """fp32 numpy inputs of both head entries on rows y [B, L, A, 128]: a DiagGaussian head with distinct log_std, actions mu + sigma eps,
    log_probs_old = logp - delta off the clip (actor_update_reference.make_old_log_probs), advantages of both signs; v_out, b_values = v - d
    with |d| in `value_bands` (off the value clip 0.1 by >= 0.05), returns on b_values' side of v (branch "orig": the unclipped mean loss is the
    larger), beyond v (branch "clip") or — branch "tie" — b_values = 0 with |v| < 0.05, so that clipped is v bit for bit."""
    g = np.random.default_rng(seed)
    f32 = np.float32
    y = g.standard_normal((B, L, A, H)).astype(f32)
    c = {"y": y, "head_w": (head_scale * g.standard_normal((4, H))).astype(f32), "head_b": (0.1 * g.standard_normal(4)).astype(f32),
         "log_std": np.array([-0.3, 0.1, 0.25, -0.1], f32)}
    mu = y.astype(np.float64) @ c["head_w"].astype(np.float64).T + c["head_b"].astype(np.float64)
    sigma = np.exp(c["log_std"].astype(np.float64))
    c["action"] = (mu + sigma * g.standard_normal(mu.shape)).astype(f32)
    z = (c["action"].astype(np.float64) - mu) / sigma
    logp = (-0.5 * z * z - np.log(sigma) - 0.5 * math.log(2 * math.pi)).sum(-1)
    c["log_probs_old"] = UA.make_old_log_probs(logp[..., None], seed + 1, bands)[..., 0]
    c["advantages"] = g.standard_normal((B, L, A)).astype(f32)
    vs = 0.0003 if branch == "tie" else head_scale
    c["v_w"], c["v_b"] = (vs * g.standard_normal((1, H))).astype(f32), np.array([0.0 if branch == "tie" else 0.2], f32)
    v = (y.astype(np.float64) @ c["v_w"].astype(np.float64).T)[..., 0] + float(c["v_b"][0])
    if branch == "tie":
        assert np.abs(v).max() < 0.05
        c["b_values"] = np.zeros((B, L, A), f32)
        c["b_returns"] = (v + g.standard_normal(v.shape)).astype(f32)
        return c
    pick = g.integers(0, len(value_bands), v.shape)
    lo, hi = np.array([b[0] for b in value_bands])[pick], np.array([b[1] for b in value_bands])[pick]
    d = (lo + (hi - lo) * g.random(v.shape)) * np.where(g.random(v.shape) < 0.5, -1.0, 1.0)
    c["b_values"] = (v - d).astype(f32)
    # returns 1 +- 0.5 away from v: towards b_values ("orig": clipping moves the value towards the return) or away from it ("clip")
    c["b_returns"] = (v + (-1.0 if branch == "orig" else 1.0) * np.sign(d) * (1.0 + 0.5 * g.random(v.shape))).astype(f32)
    return c


def gate(tag, items, bar=BAR, verbose=True):
    """items: (name, value, fp64 reference, fp32 reference) -> (worst ratio, [failures]) of e / max(e_32, 2^-24 max|ref_64|)."""
    worst, bad = 0.0, []
    for name, got, r64, r32 in items:
        h, a, b = (np.asarray(x, np.float64) for x in (got, r64, r32))
        assert h.shape == a.shape == b.shape, (name, h.shape, a.shape, b.shape)
        assert np.isfinite(h).all(), f"{tag} {name}: not finite"
        e, e32 = float(np.abs(h - a).max()), float(np.abs(b - a).max())
        bound = max(e32, 2.0 ** -24 * float(np.abs(a).max()))
        ratio = e / bound if bound > 0 else (0.0 if e == 0 else math.inf)
        if verbose:
            print(f"  {tag} {name}: e {e:.3e} e_32 {e32:.3e} max|ref| {np.abs(a).max():.3e} ratio {ratio:.2f}")
        worst = max(worst, ratio)
        if not ratio <= bar:
            bad.append(f"{name}: e {e:.3e} > {bar} x {bound:.3e} (ratio {ratio:.2f})")
    return worst, bad


# ---------------------------------------------------------------------------------------------------------------------------------------
# the whole update
def rollout_case(N, T, A, K, D, L, seed, flag_p=0.1):
    """A stored rollout for the update functions (fp32 numpy): networks with a GRU each (policy_rnn_reference.random_net), observations
    [N, T, A, ...], nonzero stored states [N, T / L, A, 128], env-level flags with one at step 0 of a segment and one in the middle of one."""
    import policy_rnn_reference as RR
    actor, critic = RR.random_net(D, A, seed)
    o, _ = R.random_obs(N * T, A, K, D, seed + 1)
    obs = {k: v.reshape(N, T, *v.shape[1:]) for k, v in o.items()}
    g = np.random.default_rng(seed + 2)
    S = T // L
    states = {w: (0.5 * g.standard_normal((N, S, A, H))).astype(np.float32) for w in ("actor", "critic")}
    is_init = g.random((N, T, 1)) < flag_p
    is_init[0, 0, 0] = True                                      # step 0 of segment 0
    is_init[N - 1, min(L // 2, T - 1), 0] = True                 # the middle of a segment
    return actor, critic, obs, states, is_init


def flow(net, actor, obs, state, is_init, per_row, seg, L, dtype, clip_param=0.1, entropy_coef=1e-3, loss="huber", huber_delta=10.0):
    """One network's update up to backward(): ({reference name: gradient}, scalars) as fp64 numpy.  net: {reference name: array}; obs
    {key: [N, T, A, ...]}; state [N, T / L, A, 128]; is_init [N, T, 1]; per_row: the actor's (action, log_probs_old, advantages) or the
    critic's (b_values, b_returns), [N, T, A, k]; seg: segment ids [B]."""
    p = {k: _t(v, dtype).requires_grad_(True) for k, v in net.items()}
    N, T = is_init.shape[:2]
    seg = np.asarray(seg, np.int64)
    B, A = len(seg), state.shape[2]
    idx = torch.as_tensor((seg[:, None] * L + np.arange(L)).reshape(-1))
    o = {k: _t(v, dtype).reshape(N * T, *v.shape[2:])[idx] for k, v in obs.items()}
    x = R.encoder(p, "encoder." if actor else "base.", o, dtype).reshape(B, L, A, H)
    cell = nn.GRUCell(H, H).to(dtype)
    cp = {n: p["rnn.cell." + n] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
    h = _t(state, dtype).reshape(-1, A, H)[torch.as_tensor(seg)]
    flags = _t(is_init, dtype).reshape(-1, L)[torch.as_tensor(seg)]
    outs = []
    for t in range(L):
        h = h * (1 - flags[:, t].reshape(B, 1, 1))
        h = torch.func.functional_call(cell, cp, (x[:, t].reshape(B * A, H), h.reshape(B * A, H))).reshape(B, A, H)
        outs.append(h)
    y = F.layer_norm(torch.stack(outs, 1) + x, (H,), p["rnn.layer_norm.weight"], p["rnn.layer_norm.bias"], 1e-5)
    rows = [_t(v, dtype).reshape(N * T, A, -1)[idx].reshape(B, L, A, -1) for v in per_row]
    if actor:
        total, scal = actor_statements(y, p["act_dist.fc_mean.weight"], p["act_dist.fc_mean.bias"], p["act_dist.log_std"], *rows, clip_param, entropy_coef)
    else:
        total, scal = critic_statements(y, p["v_out.weight"], p["v_out.bias"], *rows, clip_param, loss, huber_delta)
    total.backward()
    grads = {k: v.grad.double().numpy() for k, v in p.items()}
    scal["grad_norm"] = torch.tensor(math.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads.values())))
    return grads, _np(scal)


def per_row_case(actor, N, T, A, seed, net, obs, state, is_init, L):
    """The per-row tensors of a rollout: for the actor, actions around the recomputed mean with log_probs_old off the clip."""
    g = np.random.default_rng(seed)
    if not actor:
        return [g.standard_normal((N, T, A, 1)).astype(np.float32) * 0.3, g.standard_normal((N, T, A, 1)).astype(np.float32)]
    adv = g.standard_normal((N, T, A, 1)).astype(np.float32)
    sigma = np.exp(np.asarray(net["act_dist.log_std"], np.float64))
    action = (sigma * g.standard_normal((N, T, A, 4))).astype(np.float32)          # around 0: the mean is O(0.01) at this initialisation
    _, s = flow(net, True, obs, state, is_init, [action, np.zeros((N, T, A, 1), np.float32), adv], np.arange(N * (T // L)), L, torch.float64)
    lpo = UA.make_old_log_probs(s["log_probs"].reshape(N, T, A, 1), seed + 5)
    return [action, lpo, adv]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the predictor beside the learner (tests/learner_cases.py's shapes)
HIST, FUTURE = 10, 5


def predictor(A, seed):
    from hns_amd.tp_net import TPNet
    torch.manual_seed(seed)
    return TPNet(7 + 3 * A, 3 * FUTURE, FUTURE, 1)


def predictor_rollout(N, T, A, seed):
    """(TP_input [N, T, HIST, 7 + 3 A], TP_groundtruth [N, T, 3], TP_done [N, T, 1] all ones: N (T - FUTURE) selected windows)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, T, HIST, 7 + 3 * A, generator=g) * 0.5, torch.rand(N, T, 3, generator=g) * 2 - 1, torch.ones(N, T, 1))
