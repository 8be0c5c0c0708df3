"""Shared by test_central_learner.py (CPU) and test_hip_central_learner.py (GPU): a small MAPPO training state with the centralised critic
(critic_input: state), a rollout of it, and MAPPOPolicy.train_op's blocks driven BY HAND through the package's public calls — the policy's
value_only call on the last state, rollout_targets, update_tp, then per minibatch update_actor and update_critic_central with per-call
workspaces — which CentralCriticDeviceLearner.train_op must reproduce bit for bit.  DESIGN.md §7.20."""
import copy

import numpy as np
import torch
import torch.nn as nn

import learner_cases as LC
from hns_amd import actor_train as AT
from hns_amd import critic_train as CT
from hns_amd import gae, learner, tp_train
from hns_amd import policy as P

CFG = {**copy.deepcopy(LC.CFG), "critic_input": "state", "ppo_epochs": 2, "num_minibatches": 2}


def make_state(A, D, seed, device="cpu", tp=None):
    """{"actor", "critic": name -> Parameter under the reference's names, "tp": the predictor or None, "vn": ValueNorm1}."""
    actor, critic = P.random_parameters_central(D, A, seed)
    g = torch.Generator().manual_seed(seed + 1)
    actor["act_dist.fc_mean.weight"] = actor["act_dist.fc_mean.weight"] * 30.0
    critic["v_out.weight"] = critic["v_out.weight"] * 30.0
    for p in (actor, critic):
        for k in p:
            if k.endswith("bias"):
                p[k] = p[k] + torch.randn(p[k].shape, generator=g) * 0.1
    par = lambda d: {k: nn.Parameter(v.to(device)) for k, v in d.items()}           # noqa: E731
    return {"actor": par(actor), "critic": par(critic), "tp": tp, "vn": learner.ValueNorm1(beta=0.995).to(device)}


def clone_state(state):
    return {"actor": {k: nn.Parameter(v.detach().clone()) for k, v in state["actor"].items()},
            "critic": {k: nn.Parameter(v.detach().clone()) for k, v in state["critic"].items()},
            "tp": copy.deepcopy(state["tp"]), "vn": copy.deepcopy(state["vn"])}


def make_rollout(state, N, T, A, D, K, seed):
    """A CPU rollout without the predictor: random observations and state, the state's own policy for actions, log-probabilities and values."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                     # noqa: E731
    xs, xc, sd = r(N, T, A, 1, D) * 0.7, r(N, T, A, K, 5) * 0.5, r(N, T, A, D) * 0.7
    xo = r(N, T, A, A - 1, 3) * 0.5 if A > 1 else None
    cpu = lambda d: {k: v.detach().cpu() for k, v in d.items()}                     # noqa: E731
    pol = P.CentralCriticDevicePolicy(cpu(state["actor"]), cpu(state["critic"]), seed=seed)
    flat = lambda t: t.reshape(N * T, *t.shape[2:]) if t is not None else None      # noqa: E731
    out = pol.forward(flat(xs), flat(xo), flat(xc), flat(sd))
    return {"obs_self": xs, "obs_others": xo, "obs_cylinders": xc, "action": out.action.reshape(N, T, A, 4).contiguous(),
            "log_probs": out.log_prob.reshape(N, T, A, 1).contiguous(), "state_value": out.value.reshape(N, T, A, 1).contiguous(),
            "next_obs_last": (r(N, A, 1, D) * 0.7, r(N, A, A - 1, 3) * 0.5 if A > 1 else None, r(N, A, K, 5) * 0.5),
            "reward": r(N, T, A, 1), "done": torch.rand(N, T, 1, generator=g) < 0.1, "agent_done": None,
            "state_drones": sd, "next_state_last": r(N, A, D) * 0.7}


def as_tensordict(ro, agent="drone"):
    """The rollout as the collector's nested tensordict, with the ("agents", "state") groups a centralised critic reads."""
    from hns_amd.tensordict_shim import _ShimTensorDict
    N, T = ro["action"].shape[:2]
    stretch = lambda t: t.unsqueeze(1).expand(N, T, *t.shape[1:])                   # noqa: E731  (only [:, -1] is read)
    xs_l, xo_l, xc_l = ro["next_obs_last"]
    obs, nobs = {"state_self": ro["obs_self"], "cylinders": ro["obs_cylinders"]}, {"state_self": stretch(xs_l), "cylinders": stretch(xc_l)}
    if ro["obs_others"] is not None:
        obs["state_others"], nobs["state_others"] = ro["obs_others"], stretch(xo_l)
    td = _ShimTensorDict({}, [N, T])
    td.set(("agents", "observation"), obs)
    td.set(("agents", "state"), {"state_drones": ro["state_drones"], "cylinders": ro["obs_cylinders"]})
    td.set(("agents", "action"), ro["action"])
    td.set(f"{agent}.action_logp", ro["log_probs"])
    td.set("state_value", ro["state_value"])
    td.set(("next", "agents", "observation"), nobs)
    td.set(("next", "agents", "state"), {"state_drones": stretch(ro["next_state_last"]), "cylinders": stretch(xc_l)})
    td.set(("next", "agents", "reward"), ro["reward"])
    td.set(("next", "done"), ro["done"])
    if ro.get("tp") is not None:
        td.set(("next", "agents", "TP"), {"TP_input": ro["tp"][0], "TP_groundtruth": ro["tp"][1], "TP_done": ro["tp"][2]})
    return td


def make_learner(state, cfg=CFG, seed=0, policy=None):
    dev = next(iter(state["actor"].values())).device
    return learner.CentralCriticDeviceLearner(state["actor"], state["critic"], cfg, tp_net=state["tp"], value_normalizer=state["vn"],
                                              generator=torch.Generator(device=dev).manual_seed(seed), device_policy=policy)


def hand_optimisers(state, cfg=CFG):
    return {"actor": AT.make_optimizer(state["actor"], P.cfg_without(cfg, "critic_input")), "critic": CT.make_optimizer(state["critic"], cfg),
            "tp": tp_train.TPAdam(tp_train.parameters(state["tp"]), lr=1e-4) if state["tp"] is not None else None}


def hand_train_op(state, opts, ro, gen, cfg=CFG):
    """train_op's blocks through the public calls, one seeded generator, per-call workspaces, an `.item()` per scalar."""
    xs, xo, xc = ro["obs_self"], ro["obs_others"], ro["obs_cylinders"]
    N, T, A = ro["action"].shape[:3]
    dev = xs.device
    acfg = P.cfg_without(cfg, "critic_input")
    pol = P.CentralCriticDevicePolicy(state["actor"], state["critic"], cfg)
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
            sa = AT.update_actor(state["actor"], xs, xo, xc, ro["action"], ro["log_probs"], adv, opts["actor"], index=idx, cfg=acfg)
            sc = CT.update_critic_central(state["critic"], ro["state_drones"], xc, ro["state_value"], ret, opts["critic"], index=idx, cfg=cfg)
            for k, v in {**sa, **sc}.items():
                per[k].append(v.item())
    info.update({k: LC._mean32(v) for k, v in per.items()})
    info["advantages_mean"], info["advantages_std"] = float(adv_mean), float(adv_std)
    info["value_running_mean"] = float(state["vn"].running_mean.mean())
    return info


def state_tensors(state, opts):
    """name -> tensor of everything a train_op changes: parameters, Adam's moments and step counters, ValueNorm1's buffers."""
    out = {f"actor.{k}": v for k, v in state["actor"].items()}
    out.update({f"critic.{k}": v for k, v in state["critic"].items()})
    out.update({f"vn.{k}": v for k, v in state["vn"].named_buffers()})
    groups = {"actor": list(state["actor"].values()), "critic": list(state["critic"].values())}
    if state["tp"] is not None:
        out.update({f"tp.{k}": v for k, v in state["tp"].named_parameters()})
        groups["tp"] = tp_train.parameters(state["tp"])
    for name, opt in opts.items():
        if opt is None:
            continue
        for i, p in enumerate(groups[name]):
            for k, v in opt.state[p].items():
                out[f"{name}_opt.{i}.{k}"] = v
    return out


def learner_opts(L):
    return {"actor": L.actor_opt, "critic": L.critic_opt, "tp": L.tp_opt}


def check_train_op_equals_the_hand_loop(state, ro, cfg=CFG, calls=2):
    """`calls` train_rollout calls of a CentralCriticDeviceLearner against hand_train_op from the same start and the same generator seed:
    every parameter, Adam state and ValueNorm1 buffer bit for bit, the info row's shared keys equal as fp32."""
    a, b = clone_state(state), clone_state(state)
    dev = next(iter(state["actor"].values())).device
    L = make_learner(a, cfg, seed=11)
    opts, gen = hand_optimisers(b, cfg), torch.Generator(device=dev).manual_seed(11)
    for it in range(calls):
        got = L.train_rollout(**{k: v for k, v in ro.items()})
        want = hand_train_op(b, opts, ro, gen, cfg)
        assert set(got) == {f"drone/{k}" for k in learner.INFO_KEYS if k != "TP_loss" or state["tp"] is not None}, sorted(got)
        for k, v in want.items():
            assert np.float32(got[f"drone/{k}"]) == np.float32(v), (it, k, got[f"drone/{k}"], v)
    LC.assert_same_state(state_tensors(a, learner_opts(L)), state_tensors(b, opts), "train_rollout against the hand loop")
    changed = [k for k in a["critic"] if not torch.equal(a["critic"][k], state["critic"][k])]
    assert len(changed) >= 18, changed                          # the step moved (nearly) every critic tensor
    return L, a
