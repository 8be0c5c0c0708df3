"""The cases of the recurrent update with one actor per agent (hns_amd.rnn_train.policy_loss_and_grad_rnn_per_agent), for
tests/test_per_agent_rnn_train.py (CPU) and tests/test_hip_per_agent_rnn_train.py (MI355X).  In the manner of tests/rnn_update_cases.py:

  * CASES: (A, K, D; N, T, L; B) by tag — B shuffled segment ids, a strict subset of the rollout's N T / L, with segment 0 and the segment with
    the planted mid-segment flag among them (rnn_update_cases.minibatch);
  * `plan`: the three `_agents` ops' plans restated from the kernels' constants (named in rnn_update_cases.py beside their sources); REACH:
    what each case is there for, as predicates of its plan — a constant that changes and empties a case fails the CPU file;
  * `stacked_net`, `flow`: A genuinely different recurrent actors stacked, and the reference's statements written independently of
    hns_amd.rnn_train — one module set per agent (policy_reference.encoder, an nn.GRUCell stepped in a Python loop, LayerNorm(h + x), a
    torch.distributions head on agent a's rows), the loss over ALL rows, .backward() — in any dtype;
  * `build` / `refs`: the inputs and the fp64 and fp32 flows, computed once per case and never changed;
  * SEEDS: per case the first of 900, 901, ... (`find_seed`) at which the preconditions hold and the CPU torch path of rnn_train stays at ratio
    <= SEED_BAR = 4 on every gated item, the per-agent slices among them.  The search reads nothing from a device;
  * `items`: rnn_update_reference.gate's items, per stacked tensor AND per agent slice;
  * DEFECTS / `defect_flow`: the fp32 flow with what one plan-limited defect per padded structure would lose, double or misplace."""
import collections
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import actor_update_reference as UA
import policy_reference as R
import policy_rnn_reference as RR
import rnn_update_cases as C
import rnn_update_reference as U
from per_agent_cases import E, GEMM_OUT, I_EW, O_EWS

H = U.H
MAX_AGENTS = 7                                                   # include/hns.h: HNS_MAX_AGENTS
SEED_BAR = C.SEED_BAR

Case = C.Case
CASES = {
    "default": Case(3, 5, 35, 8, 32, 16, 11),
    "second-tile": Case(3, 5, 35, 20, 32, 16, 33),
    "widest": Case(7, 16, 24, 6, 16, 16, 5),
    "longest": Case(2, 5, 20, 70, 64, 64, 65),
    "one-step": Case(3, 5, 35, 6, 4, 1, 20),
    "one-segment": Case(3, 5, 35, 4, 16, 16, 1),
    # B from the division of the workgroups: floor(256 / 3) = 85 sweep workgroups per agent, so 85 x 16 + 1 = 1361 segments give agent a's
    # workgroup 0 a second tile (holding one sequence); 1361 x 4 = 5444 positions are 171 trips of the head against floor(512 / 3) = 170
    # workgroups per agent: workgroup 0 of every agent takes a second trip (of 4 rows).  1361 x 4 x 3 = 16 332 rows.
    "second-trip": Case(3, 5, 20, 1365, 4, 4, 1361),
}
TAGS = list(CASES)
# find_seed's results (python tests/per_agent_rnn_update_cases.py prints them)
SEEDS = {"default": 900, "second-tile": 900, "widest": 900, "longest": 900, "one-step": 900, "one-segment": 900, "second-trip": 900}


def _cdiv(a, b):
    return -(-a // b)


_up = C._up


def plan(case):
    """The plans of the three `_agents` ops for one call, as a dict (csrc/hns_gru.hip: gru_plan_agents; csrc/hns_policy_train.hip:
    ct_plan_agents / ct_plan_encoder_agents; csrc/hns_rnn_train.hip: rt_groups_per_agent, rt_actor_agents_ws)."""
    A, K, D, N, T, L, B = case
    pos = B * L                                                  # positions (b, t) of one agent
    p = {"rows": pos * A, "positions": pos, "segments": N * (T // L)}
    # the GRU's sweeps: 16-sequence tiles of ONE agent; A gpa workgroups, each one agent's for the launch
    p["gru_tpa"] = _cdiv(B, C.GRU_TILE)
    p["gru_gpa"] = min(p["gru_tpa"], C.GRU_GROUPS // A)
    p["gru_trips"] = _cdiv(p["gru_tpa"], p["gru_gpa"])
    p["gru_last_tile_seqs"] = B - C.GRU_TILE * (p["gru_tpa"] - 1)
    # its weight gradients: each agent's B L gate-gradient rows padded to spa ranges of tps 32-row tiles
    wg = _cdiv(pos, C.GRU_WG_ROWS)
    p["gru_wg_tiles"] = wg
    p["gru_tps"] = _cdiv(wg, C.GRU_SPLITS // A)
    p["gru_spa"] = _cdiv(wg, p["gru_tps"])
    p["gru_rpa"] = p["gru_spa"] * p["gru_tps"] * C.GRU_WG_ROWS
    p["gru_bytes"] = (_up(A * p["gru_rpa"] * C.GRU_GATE * 4) + _up(A * p["gru_spa"] * 6 * (H * H + H) * 4) + _up(A * p["gru_gpa"] * 2 * H * 4))
    # the encoder: 32-position tiles of ONE agent, padded to spa ranges of tps tiles
    tpa = _cdiv(pos, C.ENC_ROWS)
    p["enc_tpa"] = tpa
    p["enc_tps"] = _cdiv(tpa, max(1, C.ENC_SPLITS // A))
    p["enc_spa"] = _cdiv(tpa, p["enc_tps"])
    p["enc_padded_tpa"] = p["enc_spa"] * p["enc_tps"]
    p["enc_padding_positions"] = p["enc_padded_tpa"] * C.ENC_ROWS - pos
    img, P, P4 = I_EW + (D + 8) * E, O_EWS + D * E, O_EWS + D * E + 3 * E + 4      # ct_img_floats(D), ct_partial_floats(D, 0), (D, 4)
    tiles, splits = A * p["enc_padded_tpa"], A * p["enc_spa"]
    gblocks, tblocks = _cdiv(6 * GEMM_OUT, 32), _cdiv(P, 32)
    assert _cdiv(P4, 32) >= tblocks
    p["enc_forward_bytes"] = _up(A * img * 4)
    p["enc_bytes"] = (_up(A * img * 4) + _up(A * (gblocks + tblocks) * 8) + _up(tiles * 2 * P * 4) + _up(splits * 6 * GEMM_OUT * 4) +
                      _up(12 * tiles * C.ENC_ROWS * E * 4))
    # the head: trips of 32 positions of ONE agent; A gpa workgroups
    p["head_trips"] = _cdiv(pos, C.HEAD_ROWS)
    p["head_gpa"] = min(p["head_trips"], C.HEAD_GROUPS // A)
    p["head_last_trip_rows"] = pos - C.HEAD_ROWS * (p["head_trips"] - 1)
    p["head_bytes"] = _up(A * p["head_gpa"] * C.HEAD_SLOTS[0] * 8) + _up(pos * A * 4) + _up(L * A * 8)
    return p


# what each case reaches, as predicates of (its plan, the case): every one is asserted by test_per_agent_rnn_train.py
REACH = {
    "default": lambda p, c: p["gru_tpa"] == 1 and p["gru_last_tile_seqs"] == 11 < C.GRU_TILE and p["gru_gpa"] == 1,
    "second-tile": lambda p, c: p["gru_tpa"] == 3 and p["gru_last_tile_seqs"] == 1 and p["gru_spa"] == 17 >= 2 and p["enc_spa"] == 9 >= 2 and
    p["enc_tps"] == 2 and p["enc_padded_tpa"] == p["enc_tpa"] + 1,
    "widest": lambda p, c: c.A == MAX_AGENTS and c.K == 16 and p["gru_gpa"] == 1 and C.GRU_GROUPS // c.A == 36,
    "longest": lambda p, c: c.L == C.GRU_MAX_STEPS and p["gru_wg_tiles"] == 130 > C.GRU_SPLITS // c.A and p["gru_tps"] == 2 and p["enc_tps"] == 6 and
    p["enc_padded_tpa"] > p["enc_tpa"],
    "one-step": lambda p, c: c.L == 1 and p["gru_tpa"] == 2 and p["positions"] == 20 < C.ENC_ROWS,
    "one-segment": lambda p, c: c.B == 1 and p["gru_last_tile_seqs"] == 1 and p["gru_tpa"] == 1,
    "second-trip": lambda p, c: p["gru_tpa"] == p["gru_gpa"] + 1 == C.GRU_GROUPS // c.A + 1 and p["gru_trips"] == 2 and p["gru_last_tile_seqs"] == 1 and
    p["head_trips"] == p["head_gpa"] + 1 == C.HEAD_GROUPS // c.A + 1 and p["head_last_trip_rows"] == 4 and c.L <= 4 and c.D == 20 and c.A <= 3 and
    p["rows"] <= 20000,
}


# ---------------------------------------------------------------------------------------------------------------- the networks and the flow
def stacked_net(D, A, seed):
    """{reference name: [A, ...] fp32} — A independently initialised recurrent actors (policy_rnn_reference.random_net at A seeds), every
    agent's log_std different."""
    each = [RR.random_net(D, A, seed + 100 * (a + 1))[0] for a in range(A)]
    net = {k: np.stack([np.asarray(e[k], np.float32) for e in each]) for k in each[0]}
    net["act_dist.log_std"] = net["act_dist.log_std"] + (0.07 * np.arange(A, dtype=np.float32))[:, None]
    return net


def agent(net, a):
    return {k: v[a] for k, v in net.items()}


GRU_CELL = C.GRU_CELL
ENC_GEMM = C.ENC_GEMM


def flow(net, obs, state, is_init, per_row, seg, L, dtype, keep=None, clip_param=0.1, entropy_coef=1e-3):
    """The update of the STACKED actor up to backward(): ({reference name: gradient [A, ...]}, scalars) as fp64 numpy.  One module set per
    agent: agent a's encoder, GRUCell loop, LayerNorm(h + x) and DiagGaussian head on agent a's rows, the outputs stacked on the agent axis
    (mappo.py:281-284's vmap written as a loop), then update_actor's statements over all rows.  `keep` (defect_keep): contributions left out
    or counted twice by detaching what they would flow through — never by changing a value of the forward pass."""
    keep = keep or {}
    p = {k: U._t(v, dtype).requires_grad_(True) for k, v in net.items()}
    N, T = is_init.shape[:2]
    seg = np.asarray(seg, np.int64)
    B, A = len(seg), state.shape[2]
    idx = torch.as_tensor((seg[:, None] * L + np.arange(L)).reshape(-1))
    o = {k: U._t(v, dtype).reshape(N * T, *v.shape[2:])[idx] for k, v in obs.items()}
    h0 = U._t(state, dtype).reshape(-1, A, H)[torch.as_tensor(seg)]
    flags = U._t(is_init, dtype).reshape(-1, L)[torch.as_tensor(seg)]
    cell = nn.GRUCell(H, H).to(dtype)
    rows = [U._t(v, dtype).reshape(N * T, A, -1)[idx].reshape(B, L, A, -1) for v in per_row]
    logps, ents = [], []
    for a in range(A):
        pa = agent(p, a)
        oa = {k: v[:, a] for k, v in o.items()}
        x = R.encoder(pa, "encoder.", oa, dtype)                                  # [B L, 128]
        if "enc_dup" in keep:                                    # the rows' part of the six matrices' gradients counted twice
            lost = {k: (v.detach() if k in ["encoder." + n for n in ENC_GEMM] else v) for k, v in pa.items()}
            dup = torch.as_tensor(keep["enc_dup"][:, :, a]).to(dtype).reshape(B * L, 1)
            x = x + dup * (x - R.encoder(lost, "encoder.", oa, dtype))
        x = x.reshape(B, L, H)
        cp = {n: pa["rnn.cell." + n] for n in GRU_CELL}
        cd = {n: v.detach() for n, v in cp.items()}
        h, outs = h0[:, a], []
        for t in range(L):
            h = h * (1 - flags[:, t].reshape(B, 1))
            hn = torch.func.functional_call(cell, cp, (x[:, t], h))
            if "gru_wg" in keep:
                hn = torch.where(torch.as_tensor(keep["gru_wg"][:, a, t]).reshape(B, 1), hn, torch.func.functional_call(cell, cd, (x[:, t], h)))
            h = hn
            outs.append(h)
        y = F.layer_norm(torch.stack(outs, 1) + x, (H,), pa["rnn.layer_norm.weight"], pa["rnn.layer_norm.bias"], 1e-5)      # [B, L, 128]
        if "gru_seq" in keep:
            y = torch.where(torch.as_tensor(keep["gru_seq"][:, a]).reshape(B, 1, 1), y, y.detach())
        mean = F.linear(y, pa["act_dist.fc_mean.weight"], pa["act_dist.fc_mean.bias"])
        dist = torch.distributions.Independent(torch.distributions.Normal(mean, torch.exp(pa["act_dist.log_std"]).expand_as(mean), validate_args=False), 1,
                                               validate_args=False)
        logps.append(dist.log_prob(rows[0][:, :, a]))
        ents.append(dist.entropy())
    log_probs, dist_entropy = torch.stack(logps, 2).unsqueeze(-1), torch.stack(ents, 2).unsqueeze(-1)       # [B, L, A, 1]
    lpo, adv = rows[1], rows[2]
    ratio = torch.exp(log_probs - lpo)
    surr1 = ratio * adv
    surr2 = torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param) * adv
    policy_loss = -torch.mean(torch.min(surr1, surr2) * 4)
    entropy_loss = -torch.mean(dist_entropy)
    (policy_loss + entropy_loss * entropy_coef).backward()
    with torch.no_grad():
        ess = (2 * ratio.logsumexp(0) - (2 * ratio).logsumexp(0)).exp().mean() / ratio.shape[0]
        inside = (ratio >= 1.0 - clip_param) & (ratio <= 1.0 + clip_param)
        wgt = (inside | (surr1 < surr2)).double()
        agent_loss = (-torch.min(surr1, surr2) * 4).mean((0, 1, 3))               # [A]: each agent's own mean
        agent_entropy = dist_entropy.mean((0, 1, 3))
    grads = {k: v.grad.double().numpy() for k, v in p.items()}
    scal = {"policy_loss": policy_loss.detach(), "entropy": -entropy_loss.detach(), "ess": ess, "log_probs": log_probs.detach().squeeze(-1),
            "ratio": ratio.detach().squeeze(-1), "w": wgt.squeeze(-1), "agent_loss": agent_loss, "agent_entropy": agent_entropy,
            "grad_norm": torch.tensor(math.sqrt(sum(float((g ** 2).sum()) for g in grads.values())))}
    return grads, U._np(scal)


def per_row_case(net, N, T, A, seed, obs, state, is_init, L):
    """rnn_update_reference.per_row_case for the stacked actor: actions around 0 on each agent's scale, log_probs_old off the clip."""
    g = np.random.default_rng(seed)
    adv = g.standard_normal((N, T, A, 1)).astype(np.float32)
    sigma = np.exp(np.asarray(net["act_dist.log_std"], np.float64))               # [A, 4]
    action = (sigma * g.standard_normal((N, T, A, 4))).astype(np.float32)
    _, s = flow(net, obs, state, is_init, [action, np.zeros((N, T, A, 1), np.float32), adv], np.arange(N * (T // L)), L, torch.float64)
    return [action, UA.make_old_log_probs(s["log_probs"].reshape(N, T, A, 1), seed + 5), adv]


Built = collections.namedtuple("Built", ["case", "net", "obs", "state", "is_init", "rows", "seg", "g64", "s64", "g32", "s32"])


def build(case, seed, seg=None):
    """The inputs and both flows.  seed: the rollout's (rnn_update_reference.rollout_case: observations, states, flags) and the stacked
    actor's; seed + 1000: the per-row tensors'; seed + 2000: the minibatch's."""
    A, K, D, N, T, L, B = case
    _, _, obs, states, is_init = U.rollout_case(N, T, A, K, D, L, seed)
    net, state = stacked_net(D, A, seed), states["actor"]
    rows = per_row_case(net, N, T, A, seed + 1000, obs, state, is_init, L)
    seg = C.minibatch(case, seed + 2000) if seg is None else np.asarray(seg, np.int64)
    g64, s64 = flow(net, obs, state, is_init, rows, seg, L, torch.float64)
    g32, s32 = flow(net, obs, state, is_init, rows, seg, L, torch.float32)
    return Built(case, net, obs, state, is_init, rows, seg, g64, s64, g32, s32)


_REFS = {}


def refs(tag):
    """build() of a case of the table at its recorded seed: computed once per process, never changed."""
    if tag not in _REFS:
        _REFS[tag] = build(CASES[tag], SEEDS[tag])
    return _REFS[tag]


def preconditions(b):
    """The failures of the preconditions, as strings (none: well posed): in fp64 no ratio within U.MARGIN of 1 +- 0.1 and fp32 on the same side
    of the clip on every row."""
    bad = []
    d = np.minimum(np.abs(b.s64["ratio"] - 0.9), np.abs(b.s64["ratio"] - 1.1))
    if not d.min() >= U.MARGIN:
        bad.append(f"a ratio is {d.min():.2e} from the clip's bound")
    if not np.array_equal(b.s64["w"], b.s32["w"]):
        bad.append("fp32 takes another side of the clip on some row")
    return bad


SCALARS = ("policy_loss", "entropy", "ess", "log_probs")


def call(b, to, seg=None, live=None, **kw):
    """policy_loss_and_grad_rnn_per_agent on `b`'s inputs: (the live stacked parameters with their .grad set, the result)."""
    from hns_amd import rnn_train
    live = {k: to(v) for k, v in b.net.items()} if live is None else live
    res = rnn_train.policy_loss_and_grad_rnn_per_agent(
        live, to(b.obs["state_self"]), to(b.obs["state_others"]) if b.case.A > 1 else None, to(b.obs["cylinders"]), to(b.state), to(b.is_init),
        *(to(r) for r in b.rows), segment=to(b.seg if seg is None else seg), seq_len=b.case.L, entropy_coef=1e-3, **kw)
    return live, res


def outputs(b, live, res):
    """{name: fp64 numpy} of everything gated: each stacked gradient tensor, the scalars, log_probs, grad_norm."""
    np64 = lambda t: t.detach().cpu().double().numpy()            # noqa: E731
    out = {k: np64(live[k].grad) for k in b.net}
    for k in SCALARS:
        v = getattr(res, k)
        out[k] = np64(v.squeeze(-1) if k == "log_probs" else v)
    out["grad_norm"] = np64(res.grad_norm)
    return out


def items(b, out, r64=None, r32=None, rows=None):
    """U.gate's items of `out` against b's references (or r64 / r32: (grads, scalars)): every stacked tensor whole AND every agent's slice of
    it, then the scalars; rows: the kept minibatch positions of log_probs."""
    g64, s64 = r64 if r64 is not None else (b.g64, b.s64)
    g32, s32 = r32 if r32 is not None else (b.g32, b.s32)
    its = []
    for k in b.net:
        its.append((k, out[k], g64[k], g32[k]))
        its += [(f"{k}[{a}]", out[k][a], g64[k][a], g32[k][a]) for a in range(b.case.A)]
    for k in SCALARS + ("grad_norm",):
        got = out[k][rows] if rows is not None and k == "log_probs" else out[k]
        its.append((k, got, s64[k], s32[k]))
    return its


def find_seed(tag, start=900, tries=600, verbose=True):
    """The first seed from `start` at which the case is well posed and rnn_train's CPU torch path stays at ratio <= SEED_BAR on every item."""
    to = lambda v: torch.as_tensor(np.asarray(v)).clone()         # noqa: E731
    for seed in range(start, start + tries):
        b = build(CASES[tag], seed)
        bad = preconditions(b)
        worst = math.inf
        if not bad:
            worst, _ = U.gate(tag, items(b, outputs(b, *call(b, to))), verbose=False)
        if verbose:
            print(f"  {tag} seed {seed}: {bad or 'well posed'}, CPU path's worst ratio {worst:.2f}", flush=True)
        if not bad and worst <= SEED_BAR:
            return seed
    raise RuntimeError(f"no seed in [{start}, {start + tries}) for {tag}")


def rescaled_flow(b, keep, dtype, entropy_coef=1e-3):
    """rnn_update_cases.rescaled_flow for the stacked actor: the reference of a call whose minibatch positions outside `keep` hold
    out-of-range ids — `flow` on the kept segments at n = B L A: every gradient and mean by len(keep) / B, each agent's share
    -entropy_coef / A of the entropy term's constant gradient on log_std kept whole, the entropy unchanged, ESS by the same factor."""
    A, B = b.case.A, b.case.B
    g, s = flow(b.net, b.obs, b.state, b.is_init, b.rows, b.seg[keep], b.case.L, dtype)
    f = len(keep) / B
    g = {k: ((v + entropy_coef / A) * f - entropy_coef / A if k == "act_dist.log_std" else v * f) for k, v in g.items()}
    s = dict(s)
    s["policy_loss"], s["ess"] = s["policy_loss"] * f, s["ess"] * f
    s["grad_norm"] = np.asarray(math.sqrt(sum(float((v ** 2).sum()) for v in g.values())))
    return g, s


# ---------------------------------------------------------------------------------------------------------------- the learner's rollout
LEARNER_CFG = {"ppo_epochs": 1, "num_minibatches": 2, "use_TP_net": 0, "share_actor": False, "actor": {"rnn": {"train_seq_len": 16}},
               "critic": {"rnn": {"train_seq_len": 16}}}


def learner_rollout(case, seed):
    """(stacked actor, shared critic: {reference name: fp32 tensor}; learner_kwargs; recurrent_kwargs) on the CPU for
    PerAgentRecurrentDeviceLearner.train_rollout: `build`'s rollout with the shared recurrent critic of rollout_case beside it, random
    rewards, stored values and episode ends."""
    A, K, D, N, T, L, B = case
    b = build(case, seed)
    _, c_net, _, states, _ = U.rollout_case(N, T, A, K, D, L, seed)
    g = torch.Generator().manual_seed(seed + 3000)
    r = lambda *shape: torch.randn(*shape, generator=g)          # noqa: E731
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v))       # noqa: E731
    kw = {"obs_self": t(b.obs["state_self"]), "obs_others": t(b.obs["state_others"]) if A > 1 else None, "obs_cylinders": t(b.obs["cylinders"]),
          "action": t(b.rows[0]), "log_probs": t(b.rows[1]), "state_value": r(N, T, A, 1) * 0.3,
          "next_obs_last": (r(N, A, 1, D) * 0.7, r(N, A, A - 1, 3) * 0.5 if A > 1 else None, r(N, A, K, 5) * 0.5),
          "reward": r(N, T, A, 1), "done": torch.rand(N, T, 1, generator=g) < 0.1, "agent_done": None, "tp": None}
    rk = {"is_init": t(b.is_init), "actor_rnn_state": t(b.state), "critic_rnn_state": t(states["critic"]), "rnn_seq_len": L,
          "last_critic_rnn_state": r(N, A, H) * 0.5, "last_is_init": torch.rand(N, 1, generator=g) < 0.2}
    return {k: t(v) for k, v in b.net.items()}, {k: t(v) for k, v in c_net.items()}, kw, rk


# ---------------------------------------------------------------------------------------------------------------- defects
# One plan-limited defect per padded structure of the `_agents` kernels, as what the gradients would hold:
#   agent_last_tile_dropped  : the sweeps' tiles — the last agent's last 16-sequence tile never runs backward (a tile count short by one)
#   padding_tile_live        : the encoder's padding — the positions that pad an agent's tiles to whole row ranges count as live and alias the
#                              agent's first positions, whose rows reach the six matrices' gradients twice
#   range_to_next_agent      : the GRU's row ranges — agent a's last range of gate-gradient rows is summed into agent a + 1's slice (a < A - 1)
DEFECTS = ("agent_last_tile_dropped", "padding_tile_live", "range_to_next_agent")
# defect -> the cases the CPU file plants it at and the gate must reject it on (the structure exists at every case: each has a last tile, padding
# positions behind an agent's last one and, with A > 1, a last range; these are the small ones and those that are there for that structure)
DEFECT_TABLE = {
    "agent_last_tile_dropped": ("default", "second-tile", "one-segment", "second-trip"),
    "padding_tile_live": ("default", "second-tile", "longest"),
    "range_to_next_agent": ("default", "second-tile", "longest"),
}


def defect_keep(defect, case):
    """`flow`'s keep for the defect ("gru_seq" [B, A], "enc_dup" [B, L, A], "gru_wg" [B, A, L]); empty: the structure does not exist at this
    shape.  range_to_next_agent's "gru_wg" marks (False) the rows that move; defect_flow moves them."""
    A, K, D, N, T, L, B = case
    p = plan(case)
    b, t = np.arange(B)[:, None], np.arange(L)[None, :]
    pos = b * L + t                                              # [B, L]: an agent's position, its gate-gradient row
    if defect == "agent_last_tile_dropped":
        k = np.ones((B, A), bool)
        k[C.GRU_TILE * (p["gru_tpa"] - 1):, A - 1] = False
        return {"gru_seq": k}
    if defect == "padding_tile_live":
        dup = np.broadcast_to((pos < p["enc_padding_positions"])[:, :, None], (B, L, A)).copy()
        return {"enc_dup": dup} if dup.any() else {}
    if defect == "range_to_next_agent":
        if A < 2:
            return {}
        last = pos // (p["gru_tps"] * C.GRU_WG_ROWS) == p["gru_spa"] - 1           # [B, L]: the rows of an agent's last range
        k = np.ones((B, A, L), bool)
        k[:, :A - 1, :] = ~last[:, None, :]
        return {"gru_wg": k}
    raise KeyError(defect)


def defect_flow(b, defect, dtype=torch.float32):
    """`flow` on b's inputs with the defect planted: ({name: gradient}, scalars) as fp64 numpy."""
    keep = defect_keep(defect, b.case)
    g, s = flow(b.net, b.obs, b.state, b.is_init, b.rows, b.seg, b.case.L, dtype, keep)
    if defect == "range_to_next_agent" and keep:                 # what the rows lost lands one agent further
        full, _ = flow(b.net, b.obs, b.state, b.is_init, b.rows, b.seg, b.case.L, dtype)
        for n in GRU_CELL:
            k = "rnn.cell." + n
            g[k] = g[k] + np.roll(full[k] - g[k], 1, axis=0)
        s["grad_norm"] = np.asarray(math.sqrt(sum(float((v ** 2).sum()) for v in g.values())))
    return g, s


if __name__ == "__main__":                                      # the seed search: prints SEEDS.  Arguments: tags, or tag:first seed to try
    import sys
    found = {}
    for arg_ in (sys.argv[1:] or TAGS):
        tag_, start_ = (arg_.split(":") + [""])[:2]
        found[tag_] = find_seed(tag_, start=int(start_ or 900))
    print("SEEDS = " + repr(found))
