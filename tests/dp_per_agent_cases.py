"""Shared by tests/test_dp_per_agent_learner.py (CPU, two gloo ranks) and tests/test_hip_dp_per_agent.py (MI355X): the cases of the
data-parallel per-agent update on top of the existing helpers — actor_per_agent_reference (the plain per-agent flow),
per_agent_rnn_update_cases (the recurrent per-agent flow), rnn_update_reference (the gate, the head case), dp_rnn_reference (split, segment_ids).

  * `plain_union` / `rnn_union`: the `grads` cases — a union rollout of 3 + 5 envs x 8 steps (A 3, 2 cylinders, L 4, 2 minibatches: 96 rows
    a minibatch over both ranks), each rank's units the first minibatch of its own permutation, the union's the concatenation; SEEDS are the
    first at which the fp64 flow over the union is off the clip by MARGIN and fp32 takes the same side on every row (`find_seeds`, run on the
    CPU: python tests/dp_per_agent_cases.py);
  * `stacked_head_case` / `stacked_head_autograd`: rnn_update_reference.head_case with one head per agent — A different heads over one y, the
    actions and log_probs_old redrawn per agent's head — and the reference's statements on it in any dtype, autograd over the stacked head;
  * `plain_state` / `plain_rollout` / `rnn_rollout`: what the two learners train on in both files."""
import copy
import math

import numpy as np
import torch
import torch.nn as nn

import actor_per_agent_reference as UA
import actor_update_reference as UAS
import learner_cases as LC
import per_agent_cases as PC
import per_agent_rnn_update_cases as PCR
import rnn_update_reference as U

ENVS, T, L, A, CYL, D, M = (3, 5), 8, 4, 3, 2, 35, 2
S = T // L
GLOBAL_ROWS = 96
assert sum(n * T // M for n in ENVS) * A == GLOBAL_ROWS == sum(n * S // M for n in ENVS) * L * A
SEEDS = {"plain": 700, "rnn": 900}                               # find_seeds' results
H = U.H


def _first_minibatches(units, base):
    from hns_amd import tp_train
    return [tp_train.minibatches(u, M, torch.device("cpu"), torch.Generator().manual_seed(base + r))[0].numpy() for r, u in enumerate(units)]


# ---------------------------------------------------------------------------------------------------------------- the two unions
def plain_union(seed=None):
    """(actors, obs, action, log_probs_old, advantages: test_hip_per_agent._case over the union's 64 env-steps; the ranks' local env-step
    indices; the union's index)."""
    import test_hip_per_agent as THP                             # (its data builders; importing it starts nothing on a device)
    seed = SEEDS["plain"] if seed is None else seed
    steps = sum(ENVS) * T
    actors, obs, action, lpo, adv, _ = THP._case(steps, A, CYL, D, seed)
    local = _first_minibatches([n * T for n in ENVS], 300)
    edges = np.concatenate([[0], np.cumsum(ENVS)]) * T
    index = np.concatenate([np.asarray(s, np.int64) + int(o) for s, o in zip(local, edges[:-1])])
    return actors, obs, action, lpo, adv, local, index


def plain_part(data, rank):
    """Rank `rank`'s env-steps of `plain_union`'s data, as torch tensors: (obs_self, obs_others, obs_cylinders, action, lpo, adv, index)."""
    actors, obs, action, lpo, adv, local, _ = data
    lo, hi = int(sum(ENVS[:rank]) * T), int(sum(ENVS[:rank + 1]) * T)
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v[lo:hi]))          # noqa: E731
    return t(obs["state_self"]), t(obs["state_others"]), t(obs["cylinders"]), t(action), t(lpo), t(adv), torch.as_tensor(local[rank])


def plain_refs(data, entropy_coef=1e-3):
    actors, obs, action, lpo, adv, _, index = data
    return tuple(UA.loss_and_grad(actors, obs, action, lpo, adv, index, entropy_coef=entropy_coef, dtype=dt) for dt in (torch.float64, torch.float32))


def plain_preconditions(r64, r32):
    UAS.assert_off_the_clip(r64, 0.1, margin=U.MARGIN)
    assert np.array_equal(r64["w"], r32["w"]), "fp32 takes another side of the clip on some row"


def rnn_union(seed=None):
    """(per_agent_rnn_update_cases.build over the union's 8 envs with the union's 8 segments: the inputs and the fp64 / fp32 flows; the
    ranks' local segment ids)."""
    import dp_rnn_reference as DU
    seed = SEEDS["rnn"] if seed is None else seed
    local = _first_minibatches([n * S for n in ENVS], 300)
    seg = DU.union_segments(local, ENVS, S)
    b = PCR.build(PCR.Case(A, CYL, D, sum(ENVS), T, L, len(seg)), seed, seg=seg)
    return b, local


def rnn_part(b, local, rank):
    """Rank `rank`'s envs of the union `b`: (obs_self, obs_others, obs_cylinders, state, is_init, action, lpo, adv, segment)."""
    lo, hi = sum(ENVS[:rank]), sum(ENVS[:rank + 1])
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v[lo:hi]))          # noqa: E731
    return (t(b.obs["state_self"]), t(b.obs["state_others"]), t(b.obs["cylinders"]), t(b.state), t(b.is_init), *(t(r) for r in b.rows),
            torch.as_tensor(local[rank]))


def find_seeds(tries=200):
    found = {}
    for seed in range(700, 700 + tries):
        try:
            plain_preconditions(*plain_refs(plain_union(seed)))
        except AssertionError as e:
            print(f"  plain seed {seed}: {e}")
            continue
        found["plain"] = seed
        break
    for seed in range(900, 900 + tries):
        bad = PCR.preconditions(rnn_union(seed)[0])
        print(f"  rnn seed {seed}: {bad or 'well posed'}")
        if not bad:
            found["rnn"] = seed
            break
    return found


# ---------------------------------------------------------------------------------------------------------------- one head per agent
def stacked_head_case(B, L_, A_, seed):
    """rnn_update_reference.head_case(B, L_, A_, seed) with head_w [A, 4, 128], head_b / log_std [A, 4]: agent a's head is the case's plus a
    seeded perturbation (log_std a further 0.07 a), and action / log_probs_old are redrawn around each agent's own mean, off the clip."""
    c = dict(U.head_case(B, L_, A_, seed))
    g = np.random.default_rng(seed + 77)
    f32 = np.float32
    c["head_w"] = (c["head_w"][None] + 0.03 * g.standard_normal((A_, 4, H))).astype(f32)
    c["head_b"] = (c["head_b"][None] + 0.05 * g.standard_normal((A_, 4))).astype(f32)
    c["log_std"] = (c["log_std"][None] + 0.07 * np.arange(A_)[:, None]).astype(f32)
    mu = np.einsum("blah,aoh->blao", c["y"].astype(np.float64), c["head_w"].astype(np.float64)) + c["head_b"].astype(np.float64)
    sigma = np.exp(c["log_std"].astype(np.float64))
    c["action"] = (mu + sigma * g.standard_normal(mu.shape)).astype(f32)
    z = (c["action"].astype(np.float64) - mu) / sigma
    logp = (-0.5 * z * z - np.log(sigma) - 0.5 * math.log(2 * math.pi)).sum(-1)
    c["log_probs_old"] = UAS.make_old_log_probs(logp[..., None], seed + 78)[..., 0]
    return c


def stacked_head_autograd(case, dtype, clip_param=0.1, entropy_coef=1e-3, keep=None, global_rows=None):
    """update_actor's statements (rnn_update_reference.actor_statements') with agent a's DiagGaussian head on rows (., ., a), autograd over y
    and the stacked head: {dy, d_head_w, d_head_b, d_log_std, policy_loss, entropy, log_probs, ratio, w} as fp64 numpy.  `keep`, `global_rows`
    (dp_rnn_reference.rescale_dead's rule): only the segments `keep` are live, every mean of the loss divides by global_rows, the entropy
    term is kept whole; dy has zeros at the dead segments."""
    t = lambda k: U._t(case[k], dtype)                            # noqa: E731
    B = case["y"].shape[0]
    keep = np.arange(B) if keep is None else np.asarray(keep)
    y, w, b, ls = (t(k).requires_grad_(True) for k in ("y", "head_w", "head_b", "log_std"))
    yk = y[torch.as_tensor(keep)]
    sub = lambda k: t(k)[torch.as_tensor(keep)]                   # noqa: E731
    mean = torch.einsum("blah,aoh->blao", yk, w) + b
    dist = torch.distributions.Independent(torch.distributions.Normal(mean, torch.exp(ls).expand_as(mean), validate_args=False), 1, validate_args=False)
    log_probs = dist.log_prob(sub("action")).unsqueeze(-1)
    dist_entropy = dist.entropy().unsqueeze(-1)
    ratio = torch.exp(log_probs - sub("log_probs_old").unsqueeze(-1))
    adv = sub("advantages").unsqueeze(-1)
    surr1 = ratio * adv
    surr2 = torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param) * adv
    n = float(global_rows) if global_rows is not None else float(surr1.numel())
    policy_loss = -torch.sum(torch.min(surr1, surr2) * 4) / n
    entropy_loss = -torch.mean(dist_entropy)
    g = torch.autograd.grad(policy_loss + entropy_loss * entropy_coef, [y, w, b, ls])
    with torch.no_grad():
        inside = (ratio >= 1.0 - clip_param) & (ratio <= 1.0 + clip_param)
        wgt = (inside | (surr1 < surr2)).double()
    return U._np({"dy": g[0], "d_head_w": g[1], "d_head_b": g[2], "d_log_std": g[3], "policy_loss": policy_loss.detach(), "entropy": -entropy_loss.detach(),
                  "log_probs": log_probs.detach().squeeze(-1), "ratio": ratio.detach().squeeze(-1), "w": wgt.squeeze(-1)})


def assert_off_the_clip(a64, a32, clip_param=0.1):
    """rnn_update_reference.assert_off_the_edges' condition on the actor (the critic is not part of these cases), and fp32 on the same side."""
    d = np.minimum(np.abs(a64["ratio"] - (1 - clip_param)), np.abs(a64["ratio"] - (1 + clip_param)))
    assert d.min() >= U.MARGIN, f"a ratio is {d.min():.2e} from the clip's bound"
    assert np.array_equal(a64["w"], a32["w"]), "fp32 takes another side of the clip on some row"


def head_items(tag, out, r64, r32, names, agents):
    """rnn_update_reference.gate's items: each stacked tensor whole and per agent slice, dy / log_probs / the scalars whole."""
    its = []
    for n in names:
        its.append((f"{tag}{n}", out[n], r64[n], r32[n]))
        if n in ("d_head_w", "d_head_b", "d_log_std"):
            its += [(f"{tag}{n}[{a}]", out[n][a], r64[n][a], r32[n][a]) for a in range(agents)]
    return its


# ---------------------------------------------------------------------------------------------------------------- what the learners train on
CFG_PLAIN = {**PC.CFG, "ppo_epochs": 2, "num_minibatches": M}
CFG_RNN = {"ppo_epochs": 2, "num_minibatches": M, "TP_epochs": 1, "use_TP_net": 1, "share_actor": False, "actor": {"rnn": {"train_seq_len": L}},
           "critic": {"rnn": {"train_seq_len": L}}}


def plain_state(agents, seed):
    return PC.make_state(agents, seed)


def plain_rollout(state, N, steps, agents, seed, cylinders=CYL, tp_windows=True):
    """per_agent_cases.make_rollout with `cylinders` cylinders; tp_windows False: TP_done selects no window."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                   # noqa: E731
    from hns_amd import policy as P
    K, D_ = cylinders, LC.D
    xs, xc = r(N, steps, agents, 1, D_) * 0.7, r(N, steps, agents, K, 5) * 0.5
    xo = r(N, steps, agents, agents - 1, 3) * 0.5 if agents > 1 else None
    sl = lambda v: v.detach().cpu()[:agents]                      # noqa: E731  (a rollout of fewer agents than the state's: the refusals)
    pol = P.PerAgentDevicePolicy({k: sl(v) for k, v in state["actor"].items()}, copy.deepcopy(state["critic"]).cpu(), seed=seed)
    flat = lambda t: t.reshape(N * steps, *t.shape[2:]) if t is not None else None      # noqa: E731
    out = pol.forward(flat(xs), flat(xo), flat(xc))
    done = torch.ones(N, steps, 1) if tp_windows else torch.zeros(N, steps, 1)
    return {"obs_self": xs, "obs_others": xo, "obs_cylinders": xc, "action": out.action.reshape(N, steps, agents, 4).contiguous(),
            "log_probs": out.log_prob.reshape(N, steps, agents, 1).contiguous(), "state_value": out.value.reshape(N, steps, agents, 1).contiguous(),
            "next_obs_last": (r(N, agents, 1, D_) * 0.7, r(N, agents, agents - 1, 3) * 0.5 if agents > 1 else None, r(N, agents, K, 5) * 0.5),
            "reward": r(N, steps, agents, 1), "done": torch.rand(N, steps, 1, generator=g) < 0.1, "agent_done": None,
            "tp": (r(N, steps, LC.HIST, 7 + 3 * agents) * 0.5, torch.rand(N, steps, 3, generator=g) * 2 - 1, done)}


def rnn_nets(agents, seed):
    """(stacked recurrent actor, shared recurrent critic): {reference name: fp32 tensor}."""
    _, c_net, _, _, _ = U.rollout_case(2, L, agents, CYL, D, L, seed)
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v)).clone()            # noqa: E731
    return {k: t(v) for k, v in PCR.stacked_net(D, agents, seed).items()}, {k: t(v) for k, v in c_net.items()}


def rnn_rollout(N, steps, agents, seq, seed, tp_windows=True):
    """(learner_kwargs with the predictor's entries, recurrent_kwargs) of a stored recurrent rollout on the CPU, in the manner of
    per_agent_rnn_update_cases.learner_rollout: rollout_case's observations, states and flags, random actions, log-probabilities, rewards,
    stored values and episode ends."""
    _, _, obs, states, is_init = U.rollout_case(N, steps, agents, CYL, D, seq, seed)
    g = torch.Generator().manual_seed(seed + 3000)
    r = lambda *shape: torch.randn(*shape, generator=g)           # noqa: E731
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v))        # noqa: E731
    tp = U.predictor_rollout(N, steps, agents, seed + 17)
    kw = {"obs_self": t(obs["state_self"]), "obs_others": t(obs["state_others"]) if agents > 1 else None, "obs_cylinders": t(obs["cylinders"]),
          "action": r(N, steps, agents, 4) * 0.5, "log_probs": -3.7 + 0.2 * r(N, steps, agents, 1), "state_value": r(N, steps, agents, 1) * 0.3,
          "next_obs_last": (r(N, agents, 1, D) * 0.7, r(N, agents, agents - 1, 3) * 0.5 if agents > 1 else None, r(N, agents, CYL, 5) * 0.5),
          "reward": r(N, steps, agents, 1), "done": torch.rand(N, steps, 1, generator=g) < 0.1, "agent_done": None,
          "tp": tp if tp_windows else (tp[0], tp[1], torch.zeros_like(tp[2]))}
    rk = {"is_init": t(is_init), "actor_rnn_state": t(states["actor"]), "critic_rnn_state": t(states["critic"]), "rnn_seq_len": seq,
          "last_critic_rnn_state": r(N, agents, H) * 0.5, "last_is_init": torch.rand(N, 1, generator=g) < 0.2}
    return kw, rk


def to_device(x, dev):
    if torch.is_tensor(x):
        return x.to(dev)
    if isinstance(x, (tuple, list)):
        return tuple(to_device(v, dev) for v in x)
    if isinstance(x, dict):
        return {k: to_device(v, dev) for k, v in x.items()}
    return x


def rnn_snapshot(lrn):
    """Parameters of the three networks, the three Adam states, ValueNorm1 — as a list of tensors."""
    from hns_amd import tp_train
    out = [v.detach().clone() for v in (*lrn.actor.values(), *lrn.critic.values(), *(tp_train.parameters(lrn.tp_net) if lrn.tp_net is not None else ()))]
    for opt in (lrn.actor_opt, lrn.critic_opt, lrn.tp_opt):
        if opt is not None:
            for st in opt.state_dict()["state"].values():
                out += [st["step"].clone().to(out[0].device), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    vn = lrn.value_normalizer
    return out + ([vn.running_mean.clone(), vn.running_mean_sq.clone(), vn.debiasing_term.clone()] if vn is not None else [])


def plain_snapshot(state, lrn):
    st = LC.state_tensors(state, LC.learner_opts(lrn))
    return [st[k].detach().clone() for k in sorted(st)]


def predictor(agents, seed):
    return U.predictor(agents, seed)


def param(d):
    return {k: nn.Parameter(v) for k, v in d.items()}


if __name__ == "__main__":                                      # the seed search: prints SEEDS
    print("SEEDS = " + repr(find_seeds()))
