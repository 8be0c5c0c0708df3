"""One MAPPOPolicy.train_op (learning/mappo.py:363-475) in fp64 over GIVEN minibatch rows, from the restatements the update tests already use:
policy_reference.forward (next value), the GAE / normalisation / ValueNorm1 statements in torch.float64, the predictor by fp64 autograd and
torch.optim.Adam on a double copy, actor_update_reference / critic_update_reference for each minibatch's loss and gradients, and
clip_grad_norm_ + Adam's first statements in numpy float64.  Returns the fp64 parameters per tensor — the yardstick of
test_hip_learner.py's device-against-CPU gate."""
import copy

import numpy as np
import torch

import actor_update_reference as U
import critic_update_reference as UC
import policy_reference as R
from hns_amd import gae, tp_train

import learner_cases as LC


def clip_adam64(params, grads, ms, vs, t, norm, max_norm, lr, betas=(0.9, 0.999), eps=1e-8):
    """clip_grad_norm_ (torch's statements: max_norm / (norm + 1e-6), clamped at 1) and torch.optim.Adam's step t, float64, in place."""
    coef = min(max_norm / (norm + 1e-6), 1.0)
    b1, b2 = betas
    for k in params:
        g = grads[k] * coef
        ms[k] += (g - ms[k]) * (1 - b1)
        vs[k] = vs[k] * b2 + (1 - b2) * g * g
        denom = np.sqrt(vs[k]) / np.sqrt(1 - b2 ** t) + eps
        params[k] -= lr / (1 - b1 ** t) * ms[k] / denom


def obs_dict(xs, xo, xc):
    o = {"state_self": xs.numpy()}
    if xo is not None:
        o["state_others"] = xo.numpy()
    o["cylinders"] = xc.numpy()
    return o


def train_op64(state, ro, cfg, tp_rows, ppo_rows, margin=1e-3):
    """state: learner_cases.make_state's (CPU, untouched); ro: a CPU rollout; tp_rows / ppo_rows: the index rows in the order used.  Asserts, in
    fp64, that no minibatch row lies within `margin` of the PPO clip's bounds or of the value clip's.  Returns {name: float64 numpy} under
    learner_cases.state_tensors' names (parameters and ValueNorm1's buffers)."""
    N, T, A = ro["action"].shape[:3]
    S = N * T
    actor = {k: v.detach().double().numpy().copy() for k, v in state["actor"].items()}
    critic = {k: v.detach().double().numpy().copy() for k, v in state["critic"].named_parameters()}
    d = lambda t: t.detach().double()                            # noqa: E731
    # mappo.py:365-402
    next_value = R.forward(actor, critic, obs_dict(*ro["next_obs_last"]), dtype=torch.float64)[4]
    vn = {k: d(v).clone() for k, v in state["vn"].named_buffers()}

    def mean_var():
        den = vn["debiasing_term"].clamp(min=state["vn"].epsilon)
        mean = vn["running_mean"] / den
        return mean, (vn["running_mean_sq"] / den - mean ** 2).clamp(min=1e-2)
    mean, var = mean_var()
    values, next_value = d(ro["state_value"]) * torch.sqrt(var) + mean, next_value * torch.sqrt(var) + mean
    dones = ro["done"].unsqueeze(-1).expand(N, T, A, 1)
    adv, ret = gae._torch_gae(d(ro["reward"]), dones, values, next_value, cfg["gamma"], cfg["gae_lambda"], False)
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    w = state["vn"].beta
    vn["running_mean"] = vn["running_mean"] * w + ret.mean() * (1.0 - w)
    vn["running_mean_sq"] = vn["running_mean_sq"] * w + (ret ** 2).mean() * (1.0 - w)
    vn["debiasing_term"] = vn["debiasing_term"] * w + 1.0 * (1.0 - w)
    mean, var = mean_var()
    ret = (ret - mean) / torch.sqrt(var)
    # mappo.py:407-443
    tp = copy.deepcopy(state["tp"]).double()
    opt = torch.optim.Adam(tp.parameters(), lr=1e-4)
    x, y = tp_train.select_windows(d(ro["tp"][0]), d(ro["tp"][1]), ro["tp"][2], LC.FUTURE, 1)
    x = x.reshape(-1, *x.shape[2:])
    for row in tp_rows:
        loss = torch.nn.MSELoss()(tp(x[row]), y[row])
        opt.zero_grad()
        loss.backward()
        opt.step()
    # mappo.py:446-461
    obs = obs_dict(*(t.reshape(S, *t.shape[2:]) if t is not None else None for t in (ro["obs_self"], ro["obs_others"], ro["obs_cylinders"])))
    flat = lambda t: t.reshape(S, A, -1).numpy()                 # noqa: E731
    action, lpo, adv, bv, ret = flat(d(ro["action"])), flat(d(ro["log_probs"])), flat(adv), flat(d(ro["state_value"])), flat(ret)
    ma, va = ({k: np.zeros_like(v) for k, v in actor.items()} for _ in range(2))
    mc, vc = ({k: np.zeros_like(v) for k, v in critic.items()} for _ in range(2))
    clip = cfg["clip_param"]
    for t, row in enumerate(ppo_rows, 1):
        idx = np.asarray(row)
        ra = U.loss_and_grad(actor, obs, action, lpo, adv, idx, clip_param=clip, entropy_coef=cfg["entropy_coef"], dtype=torch.float64)
        U.assert_off_the_clip(ra, clip, margin=margin, need_all=False)
        clip_adam64(actor, ra["grads"], ma, va, t, ra["grad_norm"], cfg["max_grad_norm"], cfg["actor"]["lr"])
        rc = UC.loss_and_grad(critic, obs, bv, ret, idx, clip_param=clip, loss="huber", huber_delta=float(cfg["critic"]["huber_delta"]),
                              dtype=torch.float64)
        dist = np.abs(np.abs(rc["values"] - bv[idx]) - clip).min()
        assert dist >= margin, f"a value is {dist:.2e} from the value clip's bound"
        assert np.abs(rc["values"] - ret[idx]).max() < float(cfg["critic"]["huber_delta"]) - margin          # Huber's quadratic side throughout
        clip_adam64(critic, rc["grads"], mc, vc, t, rc["grad_norm"], cfg["max_grad_norm"], cfg["critic"]["lr"])
    out = {f"actor.{k}": v for k, v in actor.items()}
    out.update({f"critic.{k}": v for k, v in critic.items()})
    out.update({f"tp.{k}": v.detach().numpy() for k, v in tp.named_parameters()})
    out.update({f"vn.{k}": v.numpy() for k, v in vn.items()})
    return out
