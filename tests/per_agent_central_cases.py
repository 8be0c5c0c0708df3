"""Shared by test_per_agent_central_learner.py (CPU) and test_hip_per_agent_central_learner.py (GPU): central_learner_cases.py's small
training state extended to STACKED actors (share_actor: False beside critic_input: state), a rollout of it, and MAPPOPolicy.train_op's
blocks driven BY HAND through the package's public calls — the policy's value_only call on the last state, rollout_targets, update_tp, then per
minibatch update_actor_per_agent and update_critic_central with per-call workspaces — which PerAgentCentralCriticDeviceLearner.train_op must
reproduce bit for bit.  DESIGN.md §7.21."""
import numpy as np
import torch
import torch.nn as nn

import central_learner_cases as CC
import learner_cases as LC
from hns_amd import actor_train as AT
from hns_amd import critic_train as CT
from hns_amd import gae, learner, tp_train
from hns_amd import policy as P
from hns_amd.tp_net import TPNet

CFG = {**CC.CFG, "share_actor": False}
ACTOR_CFG = P.cfg_without(CFG, "critic_input")                  # what the per-agent actor's public calls take
CRITIC_CFG = P.cfg_without(CFG, "share_actor")                  # what the centralised critic's take
HIST, FUTURE = 10, 2                                            # a two-step prediction horizon: four steps hold windows

clone_state, state_tensors, learner_opts = CC.clone_state, CC.state_tensors, CC.learner_opts


def make_tp(A, seed, device="cpu"):
    torch.manual_seed(seed)
    return TPNet(7 + 3 * A, 3 * FUTURE, FUTURE, 1).to(device)


def make_state(A, D, seed, device="cpu", tp=None):
    """central_learner_cases.make_state with the stacked actor: A independently initialised actors, every tensor [A, ...]."""
    actor = P.random_parameters_per_agent(D, A, seed)[0]
    critic = P.random_parameters_central(D, A, seed)[1]
    g = torch.Generator().manual_seed(seed + 1)
    actor["act_dist.fc_mean.weight"] = actor["act_dist.fc_mean.weight"] * 30.0
    critic["v_out.weight"] = critic["v_out.weight"] * 30.0
    for p in (actor, critic):
        for k in p:
            if k.endswith("bias"):
                p[k] = p[k] + torch.randn(p[k].shape, generator=g) * 0.1
    par = lambda d: {k: nn.Parameter(v.to(device).contiguous()) for k, v in d.items()}          # noqa: E731
    return {"actor": par(actor), "critic": par(critic), "tp": tp, "vn": learner.ValueNorm1(beta=0.995).to(device)}


def make_policy(state, seed=0, cfg=CFG):
    return P.PerAgentCentralCriticDevicePolicy(state["actor"], state["critic"], cfg, seed=seed)


def make_rollout(state, N, T, A, D, K, seed, tp=False):
    """central_learner_cases.make_rollout through the new policy's CPU path; tp: the predictor's entries as learner_cases.make_rollout's."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                     # noqa: E731
    xs, xc, sd = r(N, T, A, 1, D) * 0.7, r(N, T, A, K, 5) * 0.5, r(N, T, A, D) * 0.7
    xo = r(N, T, A, A - 1, 3) * 0.5 if A > 1 else None
    cpu = lambda d: {k: v.detach().cpu() for k, v in d.items()}                     # noqa: E731
    pol = P.PerAgentCentralCriticDevicePolicy(cpu(state["actor"]), cpu(state["critic"]), seed=seed)
    flat = lambda t: t.reshape(N * T, *t.shape[2:]) if t is not None else None      # noqa: E731
    out = pol.forward(flat(xs), flat(xo), flat(xc), flat(sd))
    ro = {"obs_self": xs, "obs_others": xo, "obs_cylinders": xc, "action": out.action.reshape(N, T, A, 4).contiguous(),
          "log_probs": out.log_prob.reshape(N, T, A, 1).contiguous(), "state_value": out.value.reshape(N, T, A, 1).contiguous(),
          "next_obs_last": (r(N, A, 1, D) * 0.7, r(N, A, A - 1, 3) * 0.5 if A > 1 else None, r(N, A, K, 5) * 0.5),
          "reward": r(N, T, A, 1), "done": torch.rand(N, T, 1, generator=g) < 0.1, "agent_done": None,
          "state_drones": sd, "next_state_last": r(N, A, D) * 0.7}
    if tp:
        ro["tp"] = (r(N, T, HIST, 7 + 3 * A) * 0.5, torch.rand(N, T, 3, generator=g) * 2 - 1, torch.ones(N, T, 1))
    return ro


def make_learner(state, cfg=CFG, seed=0, policy=None):
    dev = next(iter(state["actor"].values())).device
    return learner.PerAgentCentralCriticDeviceLearner(state["actor"], state["critic"], cfg, tp_net=state["tp"], value_normalizer=state["vn"],
                                                      generator=torch.Generator(device=dev).manual_seed(seed), device_policy=policy)


def hand_optimisers(state):
    return {"actor": AT.make_optimizer_per_agent(state["actor"], ACTOR_CFG), "critic": CT.make_optimizer(state["critic"], CRITIC_CFG),
            "tp": tp_train.TPAdam(tp_train.parameters(state["tp"]), lr=1e-4) if state["tp"] is not None else None}


def hand_train_op(state, opts, ro, gen, cfg=CFG):
    """train_op's blocks through the public calls, one seeded generator, per-call workspaces, an `.item()` per scalar."""
    xs, xo, xc = ro["obs_self"], ro["obs_others"], ro["obs_cylinders"]
    N, T, A = ro["action"].shape[:3]
    dev = xs.device
    pol = make_policy(state)
    with torch.no_grad():
        next_value = pol.forward(*ro["next_obs_last"], ro["next_state_last"], value_only=True).value
    dones = ro["done"].unsqueeze(-1).expand(N, T, A, 1).contiguous()
    adv, ret, _, (adv_mean, adv_std) = gae.rollout_targets(ro["reward"], dones, ro["state_value"], next_value, cfg["gamma"], cfg["gae_lambda"],
                                                           value_normalizer=state["vn"], return_moments=True)
    info = {}
    if state["tp"] is not None:
        tp = state["tp"]
        info["TP_loss"] = float(tp_train.update_tp(tp, *ro["tp"], tp.future_predcition_step, tp.window_step, cfg["num_minibatches"], cfg["TP_epochs"],
                                                   opts["tp"], generator=gen))
    per = {k: [] for k in learner.COLUMNS}
    for _ in range(cfg["ppo_epochs"]):
        for idx in tp_train.minibatches(N * T, cfg["num_minibatches"], dev, gen):
            sa = AT.update_actor_per_agent(state["actor"], xs, xo, xc, ro["action"], ro["log_probs"], adv, opts["actor"], index=idx, cfg=ACTOR_CFG)
            sc = CT.update_critic_central(state["critic"], ro["state_drones"], xc, ro["state_value"], ret, opts["critic"], index=idx, cfg=CRITIC_CFG)
            for k, v in {**sa, **sc}.items():
                per[k].append(v.item())
    info.update({k: LC._mean32(v) for k, v in per.items()})
    info["advantages_mean"], info["advantages_std"] = float(adv_mean), float(adv_std)
    info["value_running_mean"] = float(state["vn"].running_mean.mean())
    return info


def check_train_op_equals_the_hand_loop(state, ro, cfg=CFG, calls=2):
    """`calls` train_rollout calls of a PerAgentCentralCriticDeviceLearner against hand_train_op from the same start and the same generator
    seed: every parameter, Adam state, predictor tensor and ValueNorm1 buffer bit for bit, the info row's shared keys equal as fp32."""
    a, b = clone_state(state), clone_state(state)
    dev = next(iter(state["actor"].values())).device
    L = make_learner(a, cfg, seed=11)
    opts, gen = hand_optimisers(b), torch.Generator(device=dev).manual_seed(11)
    for it in range(calls):
        got = L.train_rollout(**ro)
        want = hand_train_op(b, opts, ro, gen, cfg)
        assert set(got) == {f"drone/{k}" for k in learner.INFO_KEYS if k != "TP_loss" or state["tp"] is not None}, sorted(got)
        for k, v in want.items():
            assert np.float32(got[f"drone/{k}"]) == np.float32(v), (it, k, got[f"drone/{k}"], v)
    LC.assert_same_state(state_tensors(a, learner_opts(L)), state_tensors(b, opts), "train_rollout against the hand loop")
    for net, least in (("actor", 20), ("critic", 18)):           # the steps moved (nearly) every tensor of both networks
        changed = [k for k in a[net] if not torch.equal(a[net][k], state[net][k])]
        assert len(changed) >= least, (net, changed)
    return L, a
