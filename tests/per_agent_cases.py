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


def check_info(info, hand, use_tp=True):
    """The learner's info row against the hand-driven one: the same floats (the column means are one fp64 sum rounded once on both sides)."""
    keys = [k for k in learner.INFO_KEYS if k != "action_norm" and (use_tp or k != "TP_loss")]
    bad = [(k, info.get(f"drone/{k}"), hand.get(k)) for k in keys if k in hand and np.float32(info[f"drone/{k}"]) != np.float32(hand[k])]
    assert not bad, bad
