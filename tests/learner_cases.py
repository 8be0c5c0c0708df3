"""Shared by test_learner.py and test_hip_learner.py: a small MAPPO training state (actor parameters, a plain-torch critic of the reference's
shapes, the predictor, ValueNorm1), a rollout of it, and MAPPOPolicy.train_op's blocks driven BY HAND through the package's public calls —
rollout_targets, update_tp, then per minibatch update_actor and update_critic with per-call workspaces — which DeviceLearner.train_op must
reproduce bit for bit."""
import copy

import numpy as np
import torch
import torch.nn as nn

from hns_amd import actor_train as AT
from hns_amd import critic_train as CT
from hns_amd import gae, learner, tp_train
from hns_amd import policy as P
from hns_amd.tp_net import TPNet

K, D, HIST, FUTURE = 5, 35, 10, 5
CFG = {"ppo_epochs": 2, "num_minibatches": 4, "TP_epochs": 1, "use_TP_net": 1, "clip_param": 0.1, "entropy_coef": 0.001, "gamma": 0.995,
       "gae_lambda": 0.95, "max_grad_norm": 10.0, "normalize_advantages": True, "share_actor": True, "critic_input": "obs",
       "actor": {"lr": 5e-4, "weight_decay": 0.0, "tanh": False}, "critic": {"lr": 5e-4, "weight_decay": 0.0, "use_huber_loss": True, "huber_delta": 10}}


class _SplitEmbed(nn.Module):
    def __init__(self, A):
        super().__init__()
        dims = {"state_self": D, "state_others": 3, "cylinders": 5} if A > 1 else {"state_self": D, "cylinders": 5}
        self.embed = nn.ModuleDict({k: nn.Linear(i, P.EMBED_DIM) for k, i in dims.items()})
        self.layer_norm = nn.LayerNorm(P.EMBED_DIM)


class _Encoder(nn.Module):
    def __init__(self, A):
        super().__init__()
        E = P.EMBED_DIM
        self.split_embed = _SplitEmbed(A)
        self.attn = nn.MultiheadAttention(E, 1, batch_first=True)
        self.linear1, self.linear2 = nn.Linear(E, E), nn.Linear(E, E)
        self.norm1, self.norm2 = nn.LayerNorm(E), nn.LayerNorm(E)


class PlainCritic(nn.Module):
    """A plain torch.nn module with the parameter names and shapes of the reference's critic (make_critic over a PartialAttentionEncoder)."""

    def __init__(self, A):
        super().__init__()
        self.base = _Encoder(A)
        self.v_out = nn.Linear(P.EMBED_DIM, 1)


def make_state(A, seed, device="cpu"):
    """{"actor": name -> Parameter, "critic": PlainCritic, "tp": TPNet, "vn": ValueNorm1} from seeded initialisers."""
    actor, critic = P.random_parameters(D, A, seed)
    g = torch.Generator().manual_seed(seed + 1)
    actor["act_dist.fc_mean.weight"] = actor["act_dist.fc_mean.weight"] * 30.0          # means of order 0.3, as test_hip_actor_train.py
    for k in actor:
        if k.endswith("bias"):
            actor[k] = actor[k] + torch.randn(actor[k].shape, generator=g) * 0.1
    mod = PlainCritic(A)
    mod.load_state_dict(critic)
    torch.manual_seed(seed + 2)
    tp = TPNet(7 + 3 * A, 3 * FUTURE, FUTURE, 1)
    vn = learner.ValueNorm1(beta=0.995)
    return {"actor": {k: nn.Parameter(v.to(device)) for k, v in actor.items()}, "critic": mod.to(device), "tp": tp.to(device), "vn": vn.to(device)}


def clone_state(state, device=None):
    out = copy.deepcopy(state)
    if device is not None:
        out = {"actor": {k: nn.Parameter(v.detach().to(device)) for k, v in out["actor"].items()}, "critic": out["critic"].to(device),
               "tp": out["tp"].to(device), "vn": out["vn"].to(device)}
    return out


def make_rollout(state, N, T, A, seed):
    """A CPU rollout of the state's own policy (actions, log-probabilities and values are its forward pass), random rewards, a tenth of the
    env-steps done, and the predictor's entries with TP_done all ones: the reference's `view(batch, -1, ...)` of the selected windows
    (mappo.py:419) needs the same count in every env, which all-ones gives."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                     # noqa: E731
    xs, xc = r(N, T, A, 1, D) * 0.7, r(N, T, A, K, 5) * 0.5
    xo = r(N, T, A, A - 1, 3) * 0.5 if A > 1 else None
    pol = P.DevicePolicy({k: v.detach().cpu() for k, v in state["actor"].items()}, copy.deepcopy(state["critic"]).cpu(), seed=seed)
    flat = lambda t: t.reshape(N * T, *t.shape[2:]) if t is not None else None      # noqa: E731
    out = pol.forward(flat(xs), flat(xo), flat(xc))
    ro = {"obs_self": xs, "obs_others": xo, "obs_cylinders": xc, "action": out.action.reshape(N, T, A, 4).contiguous(),
          "log_probs": out.log_prob.reshape(N, T, A, 1).contiguous(), "state_value": out.value.reshape(N, T, A, 1).contiguous(),
          "next_obs_last": (r(N, A, 1, D) * 0.7, r(N, A, A - 1, 3) * 0.5 if A > 1 else None, r(N, A, K, 5) * 0.5),
          "reward": r(N, T, A, 1), "done": torch.rand(N, T, 1, generator=g) < 0.1, "agent_done": None,
          "tp": (r(N, T, HIST, 7 + 3 * A) * 0.5, torch.rand(N, T, 3, generator=g) * 2 - 1, torch.ones(N, T, 1))}
    return ro


def to_device(ro, device):
    mv = lambda t: t.to(device) if torch.is_tensor(t) else (tuple(mv(x) for x in t) if isinstance(t, tuple) else t)   # noqa: E731
    return {k: mv(v) for k, v in ro.items()}


def as_tensordict(ro, agent="drone"):
    """The rollout as the collector's nested tensordict (the package's stand-in class when tensordict is not installed)."""
    from hns_amd.tensordict_shim import _ShimTensorDict
    N, T = ro["action"].shape[:2]
    obs = {"state_self": ro["obs_self"], "cylinders": ro["obs_cylinders"]}
    xs_l, xo_l, xc_l = ro["next_obs_last"]
    stretch = lambda t: t.unsqueeze(1).expand(N, T, *t.shape[1:])                   # noqa: E731  (only [:, -1] is read)
    nobs = {"state_self": stretch(xs_l), "cylinders": stretch(xc_l)}
    if ro["obs_others"] is not None:
        obs["state_others"], nobs["state_others"] = ro["obs_others"], stretch(xo_l)
    td = _ShimTensorDict({}, [N, T])
    td.set(("agents", "observation"), obs)
    td.set(("agents", "action"), ro["action"])
    td.set(f"{agent}.action_logp", ro["log_probs"])
    td.set("state_value", ro["state_value"])
    td.set(("next", "agents", "observation"), nobs)
    td.set(("next", "agents", "reward"), ro["reward"])
    td.set(("next", "done"), ro["done"])
    td.set(("next", "agents", "TP"), {"TP_input": ro["tp"][0], "TP_groundtruth": ro["tp"][1], "TP_done": ro["tp"][2]})
    return td


def make_learner(state, cfg=CFG, seed=0, use_tp=True):
    dev = next(iter(state["actor"].values())).device
    gen = torch.Generator(device=dev).manual_seed(seed)
    return learner.DeviceLearner(state["actor"], state["critic"], cfg, tp_net=state["tp"] if use_tp else None, value_normalizer=state["vn"],
                                 generator=gen)


def hand_optimisers(state, cfg=CFG):
    return {"actor": AT.make_optimizer(state["actor"], cfg), "critic": CT.make_optimizer(state["critic"], cfg),
            "tp": tp_train.TPAdam(tp_train.parameters(state["tp"]), lr=1e-4)}


def _mean32(values):
    s = 0.0
    for v in values:                                             # the fp64 sum in row order, divided once, rounded once
        s += float(v)
    return float(np.float32(s / len(values)))


def hand_train_op(state, opts, ro, gen, cfg=CFG, use_tp=True, trace=None):
    """train_op's blocks through the public calls of the parent modules, one seeded generator, per-call workspaces, an `.item()` per scalar.
    `trace` (a list) receives ("tp" | "ppo", index row) in the order drawn."""
    xs, xo, xc = ro["obs_self"], ro["obs_others"], ro["obs_cylinders"]
    N, T, A = ro["action"].shape[:3]
    dev = xs.device
    pol = P.DevicePolicy(state["actor"], state["critic"], cfg)
    with torch.no_grad():
        next_value = pol.forward(*ro["next_obs_last"], value_only=True).value
    dones = ro["done"].unsqueeze(-1).expand(N, T, A, 1).contiguous()       # mappo.py:355-360 spelled out: env_done expanded over the agents
    adv, ret, _, (adv_mean, adv_std) = gae.rollout_targets(ro["reward"], dones, ro["state_value"], next_value, cfg["gamma"], cfg["gae_lambda"],
                                                           value_normalizer=state["vn"], return_moments=True)
    info = {}
    if use_tp:
        before = gen.get_state().clone()
        info["TP_loss"] = float(tp_train.update_tp(state["tp"], *ro["tp"], FUTURE, 1, cfg["num_minibatches"], cfg["TP_epochs"], opts["tp"],
                                                   generator=gen))
        if trace is not None:                                    # the rows update_tp drew, from a copy of the generator
            g2 = torch.Generator(device=dev)
            g2.set_state(before)
            rows = N * (T - FUTURE)
            for _ in range(cfg["TP_epochs"]):
                trace += [("tp", r.tolist()) for r in tp_train.minibatches(rows, cfg["num_minibatches"], dev, g2)]
    per = {k: [] for k in learner.COLUMNS}
    for _ in range(cfg["ppo_epochs"]):
        for idx in tp_train.minibatches(N * T, cfg["num_minibatches"], dev, gen):
            if trace is not None:
                trace.append(("ppo", idx.tolist()))
            sa = AT.update_actor(state["actor"], xs, xo, xc, ro["action"], ro["log_probs"], adv, opts["actor"], index=idx, cfg=cfg)
            sc = CT.update_critic(state["critic"], xs, xo, xc, ro["state_value"], ret, opts["critic"], index=idx, cfg=cfg)
            for k, v in {**sa, **sc}.items():
                per[k].append(v.item())
    info.update({k: _mean32(v) for k, v in per.items()})
    info["advantages_mean"], info["advantages_std"] = float(adv_mean), float(adv_std)
    a64 = ro["action"].detach().cpu().reshape(-1, 4).double().numpy()
    info["action_norm_f64"] = float(np.sqrt((a64 * a64).sum(-1)).sum() / a64.shape[0])          # the unrounded fp64 value
    info["value_running_mean"] = float(state["vn"].running_mean.mean())
    return info


def state_tensors(state, opts):
    """name -> tensor of everything a train_op changes: parameters, Adam's moments and step counters, ValueNorm1's buffers."""
    out = {f"actor.{k}": v for k, v in state["actor"].items()}
    out.update({f"critic.{k}": v for k, v in state["critic"].named_parameters()})
    out.update({f"tp.{k}": v for k, v in state["tp"].named_parameters()})
    out.update({f"vn.{k}": v for k, v in state["vn"].named_buffers()})
    groups = {"actor": list(state["actor"].values()), "critic": list(state["critic"].parameters()), "tp": tp_train.parameters(state["tp"])}
    for name, opt in opts.items():
        if opt is None:
            continue
        for i, p in enumerate(groups[name]):
            for k, v in opt.state[p].items():
                out[f"{name}_opt.{i}.{k}"] = v
    return out


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                      b.view(torch.int32) if b.dtype == torch.float32 else b)


def assert_same_state(got, want, what=""):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    bad = [k for k in want if not bits_equal(got[k], want[k])]
    assert not bad, f"{what}: {len(bad)} of {len(want)} tensors differ in their bits: {bad[:8]}"


def learner_opts(L):
    return {"actor": L.actor_opt, "critic": L.critic_opt, "tp": L.tp_opt}
