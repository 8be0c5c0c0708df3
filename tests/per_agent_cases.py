"""Shared by test_per_agent.py and test_hip_per_agent.py: a small MAPPO training state with ONE ACTOR PER AGENT (learner_cases' state with the
actor stacked over genuinely different agents), a rollout of it, and train_op's blocks driven BY HAND through the package's public calls —
rollout_targets, update_tp, then per minibatch update_actor_per_agent and update_critic with per-call workspaces — which
PerAgentDeviceLearner.train_rollout must reproduce bit for bit."""
import copy

import numpy as np
import torch
import torch.nn as nn

import actor_per_agent_reference as UA
import learner_cases as LC
from hns_amd import actor_train as AT
from hns_amd import critic_train as CT
from hns_amd import gae, learner, tp_train
from hns_amd import policy as P

CFG = {**LC.CFG, "share_actor": False, "num_minibatches": 2}
SHARED_CFG = {k: v for k, v in CFG.items() if k != "share_actor"}


def make_state(A, seed, device="cpu"):
    """learner_cases.make_state with "actor" the stacked actor: name -> Parameter [A, ...], every agent's slice different."""
    state = LC.make_state(A, seed)
    stacked = UA.stacked_actor({k: v.detach().numpy() for k, v in state["actor"].items()}, A, seed + 5)
    state["actor"] = {k: nn.Parameter(torch.as_tensor(v)) for k, v in stacked.items()}
    return clone_state(state, device)


def clone_state(state, device=None):
    return LC.clone_state(state, device if device is not None else next(iter(state["actor"].values())).device)


def make_rollout(state, N, T, A, seed):
    """learner_cases.make_rollout with the state's own per-agent policy."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                     # noqa: E731
    K, D = LC.K, LC.D
    xs, xc = r(N, T, A, 1, D) * 0.7, r(N, T, A, K, 5) * 0.5
    xo = r(N, T, A, A - 1, 3) * 0.5 if A > 1 else None
    pol = P.PerAgentDevicePolicy({k: v.detach().cpu() for k, v in state["actor"].items()}, copy.deepcopy(state["critic"]).cpu(), seed=seed)
    flat = lambda t: t.reshape(N * T, *t.shape[2:]) if t is not None else None      # noqa: E731
    out = pol.forward(flat(xs), flat(xo), flat(xc))
    return {"obs_self": xs, "obs_others": xo, "obs_cylinders": xc, "action": out.action.reshape(N, T, A, 4).contiguous(),
            "log_probs": out.log_prob.reshape(N, T, A, 1).contiguous(), "state_value": out.value.reshape(N, T, A, 1).contiguous(),
            "next_obs_last": (r(N, A, 1, D) * 0.7, r(N, A, A - 1, 3) * 0.5 if A > 1 else None, r(N, A, K, 5) * 0.5),
            "reward": r(N, T, A, 1), "done": torch.rand(N, T, 1, generator=g) < 0.1, "agent_done": None,
            "tp": (r(N, T, LC.HIST, 7 + 3 * A) * 0.5, torch.rand(N, T, 3, generator=g) * 2 - 1, torch.ones(N, T, 1))}


def make_learner(state, cfg=CFG, seed=0, use_tp=True):
    dev = next(iter(state["actor"].values())).device
    return learner.PerAgentDeviceLearner(state["actor"], state["critic"], cfg, tp_net=state["tp"] if use_tp else None, value_normalizer=state["vn"],
                                         generator=torch.Generator(device=dev).manual_seed(seed))


def hand_optimisers(state, cfg=CFG):
    return {"actor": AT.make_optimizer_per_agent(state["actor"], cfg), "critic": CT.make_optimizer(state["critic"], SHARED_CFG),
            "tp": tp_train.TPAdam(tp_train.parameters(state["tp"]), lr=1e-4)}


def hand_train_op(state, opts, ro, gen, cfg=CFG, use_tp=True):
    """learner_cases.hand_train_op with the per-agent policy and update_actor_per_agent in the actor's place."""
    xs, xo, xc = ro["obs_self"], ro["obs_others"], ro["obs_cylinders"]
    N, T, A = ro["action"].shape[:3]
    dev = xs.device
    pol = P.PerAgentDevicePolicy(state["actor"], state["critic"], cfg)
    with torch.no_grad():
        next_value = pol.forward(*ro["next_obs_last"], value_only=True).value
    dones = ro["done"].unsqueeze(-1).expand(N, T, A, 1).contiguous()
    adv, ret, _, (adv_mean, adv_std) = gae.rollout_targets(ro["reward"], dones, ro["state_value"], next_value, cfg["gamma"], cfg["gae_lambda"],
                                                           value_normalizer=state["vn"], return_moments=True)
    info = {}
    if use_tp:
        info["TP_loss"] = float(tp_train.update_tp(state["tp"], *ro["tp"], LC.FUTURE, 1, cfg["num_minibatches"], cfg["TP_epochs"], opts["tp"],
                                                   generator=gen))
    per = {k: [] for k in learner.COLUMNS}
    for _ in range(cfg["ppo_epochs"]):
        for idx in tp_train.minibatches(N * T, cfg["num_minibatches"], dev, gen):
            sa = AT.update_actor_per_agent(state["actor"], xs, xo, xc, ro["action"], ro["log_probs"], adv, opts["actor"], index=idx, cfg=cfg)
            sc = CT.update_critic(state["critic"], xs, xo, xc, ro["state_value"], ret, opts["critic"], index=idx, cfg=SHARED_CFG)
            for k, v in {**sa, **sc}.items():
                per[k].append(v.item())
    info.update({k: LC._mean32(v) for k, v in per.items()})
    info["advantages_mean"], info["advantages_std"] = float(adv_mean), float(adv_std)
    info["value_running_mean"] = float(state["vn"].running_mean.mean())
    return info


# ---------------------------------------------------------------------------------------------------------------- the padded plan
# csrc/hns_policy_train.hip restated: kCtRows, kCtMaxSplits, kCtE, kCtMat, kCtGemmOut, kActLossSlots (1 + 3 HNS_MAX_AGENTS), I_EW, O_EWS, kActDim
ROWS, MAX_SPLITS, E, ACT = 32, 48, 128, 4
MAT, LOSS_SLOTS, I_EW, O_EWS = E * E, 1 + 3 * 7, 12 * E * E, 1280 + 3 * E + 5 * E + 4
GEMM_OUT = MAT + E


def agents_plan(B, A):
    """ct_plan_agents for B minibatch positions of each of A agents: (tiles per agent, tiles per row range of the weight-gradient kernel,
    row ranges per agent, padding tiles per agent, tiles in all)."""
    tpa = -(-B // ROWS)
    spa = max(1, MAX_SPLITS // A)
    tps = -(-tpa // spa)
    spa = -(-tpa // tps)
    return tpa, tps, spa, spa * tps - tpa, A * spa * tps


def agents_workspace_bytes(B, D, A, K):
    """hns_actor_train_agents_workspace_bytes(B A, D, A, K): ct_plan_agents' sum of 256-byte aligned arrays — the control floats, the tiles' loss
    partials (fp64), the agents' per-block sums (fp64), the A packed images, two partial rows per tile, six weight-gradient partials per row
    range, twelve staged operand arrays of 32 rows per tile."""
    up = lambda v: (v + 255) & ~255                                                 # noqa: E731
    _, _, spa, _, tiles = agents_plan(B, A)
    P = O_EWS + D * E + (ACT - 1) * E + ACT                                         # ct_partial_floats(D, kActDim)
    img = I_EW + (D + 8) * E                                                        # ct_img_floats(D)
    gblocks, tblocks = (6 * GEMM_OUT + 31) // 32, (P + 31) // 32
    return (up(64 * 4) + up(tiles * LOSS_SLOTS * 8) + up(A * (gblocks + tblocks) * 8) + up(A * img * 4) + up(tiles * 2 * P * 4) +
            up(A * spa * 6 * GEMM_OUT * 4) + up(12 * tiles * ROWS * E * 4))


# (A, K, D, S, B) -> (tpa, tps, spa, padding tiles per agent, tiles): the smallest shapes that reach each mechanism of the padded plan.  B None:
# no index, the rollout's S env-steps read in place
EDGE_PLANS = {
    (7, 16, 24, 200, 192): (6, 1, 6, 0, 42),       # the last B at tps = 1 for A = 7
    (7, 16, 24, 200, 193): (7, 2, 4, 1, 56),       # first tps = 2; a one-row last live tile next to a padding tile in one range
    (7, 16, 24, 260, 256): (8, 2, 4, 0, 56),       # tps = 2, exact fit
    (7, 16, 24, 400, 385): (13, 3, 5, 2, 105),     # tps = 3, two padding tiles in the last range, the loss merge's second trip (105 > 64)
    (5, 8, 20, 330, 321): (11, 2, 6, 1, 60),       # an A whose 48 / A is not exact
    (3, 5, 35, 520, 513): (17, 2, 9, 1, 54),       # the default shape's A, K, D
    (2, 8, 20, 780, 769): (25, 2, 13, 1, 52),
    (1, 5, 20, 1540, 1537): (49, 2, 25, 1, 50),    # A = 1, no state_others
    (3, 5, 35, 513, None): (17, 2, 9, 1, 54),      # no index
}
EDGE_CASES = list(EDGE_PLANS)
EXACT_FIT = [(7, 16, 24, 200, 192), (7, 16, 24, 260, 256)]
# The seed of a case is test_hip_per_agent._case's 500 + A + S, but for the four cases whose seed leaves some agent's ONE-row last live tile a
# clipped row (w = 0: zero gradient, so a kernel that dropped the tile would show nothing; agents 1 and 4 at (7; 193), agent 0 at (7; 385),
# agent 1 at (2; 769), the agent of (1; 1537)): there the first seed 500 + A + S + 1000 k, k = 1, 2, .., that is off the clip, has w equal in
# fp64 and fp32 and gives every agent's last live tile a row with w = 1 and a non-zero advantage.  k (below) was found from the log-probabilities
# of the fp64 / fp32 references alone, before anything ran on a device; tests/test_per_agent_edges.py re-asserts all three for every case
EDGE_SEEDS = {(7, 16, 24, 200, 193): 500 + 7 + 200 + 1000 * 6, (7, 16, 24, 400, 385): 500 + 7 + 400 + 1000 * 13,
              (2, 8, 20, 780, 769): 500 + 2 + 780 + 1000 * 1, (1, 5, 20, 1540, 1537): 500 + 1 + 1540 + 1000 * 1}


def edge_tag(case):
    A, K, D, S, B = case
    return f"a{A}k{K}d{D}-s{S}b{B if B else 'all'}"


def edge_positions(case):
    """The positions per agent of a case's minibatch."""
    return case[4] if case[4] else case[3]


def edge_case(case):
    """(actors, obs, action, log_probs_old, advantages, index) of test_hip_per_agent._case at the case's seed."""
    import test_hip_per_agent as THP                             # (its data builders; importing it starts nothing on a device)
    A, K, D, S, B = case
    return THP._case(S, A, K, D, EDGE_SEEDS.get(case, 500 + A + S), B=B)


def check_info(info, hand, use_tp=True):
    """The learner's info row against the hand-driven one: the same floats (the column means are one fp64 sum rounded once on both sides)."""
    keys = [k for k in learner.INFO_KEYS if k != "action_norm" and (use_tp or k != "TP_loss")]
    bad = [(k, info.get(f"drone/{k}"), hand.get(k)) for k in keys if k in hand and np.float32(info[f"drone/{k}"]) != np.float32(hand[k])]
    assert not bad, bad
