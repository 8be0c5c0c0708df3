"""learner.RecurrentDeviceLearner on an MI355X: one train_rollout on the device equals the hand-driven sequence of public
calls with per-call workspaces bit for bit — parameters, the Adam states, ValueNorm1 the predictor and its TPAdam state, and the info row with TP_loss — at [8 envs, 32 steps, 3 agents] with
2 minibatches and at [5, 16, 3] with 2 minibatches, where one of the five segments is dropped; the PPO loop runs under
torch.cuda.set_sync_debug_mode("error"); a learner whose workspaces regrow equals a fresh one; the example's --learner mode.

The rollouts are collected on the CPU (the example's stand-in env behind DeviceCollector and a RecurrentDevicePolicy) and moved to the device:
the learner takes tensors, wherever they were collected."""
import copy
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rnn_update_reference as U
from hns_amd import collector, gae, learner, rnn_train, tp_train
from hns_amd import policy as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 16
CFG = {"ppo_epochs": 2, "num_minibatches": 2, "TP_epochs": 2, "use_TP_net": 1, "actor": {"rnn": {"train_seq_len": L}}, "critic": {"rnn": {"train_seq_len": L}}}


def _example():
    spec = importlib.util.spec_from_file_location("recurrent_policy_example", os.path.join(ROOT, "examples", "recurrent_policy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _to(x, dev):
    if torch.is_tensor(x):
        return x.to(dev)
    if isinstance(x, (tuple, list)):
        return tuple(_to(v, dev) for v in x)
    return x


_ROLLOUTS = {}


def _rollout(N, T):
    """(initial actor / critic parameters on the CPU, learner_kwargs, recurrent_kwargs on the device), collected once per shape."""
    if (N, T) not in _ROLLOUTS:
        ex = _example()
        torch.manual_seed(N * 100 + T)
        env = ex.StandInEnv(N, max_episode_length=11)             # episodes end inside the segments: flags in their middle
        actor, critic = ex.Network(env.D, env.A, True, 0), ex.Network(env.D, env.A, False, 1)
        pol = P.RecurrentDevicePolicy(actor.names(), critic.names(), seed=0)
        col = collector.DeviceCollector(env, pol, T, rnn_seq_len=L)
        col.collect()
        st = col.collect()                                       # the second rollout: every segment starts from a carried state
        kw, rk = {**st.learner_kwargs(), "tp": U.predictor_rollout(N, T, 3, N + T)}, st.recurrent_kwargs()
        assert rk["is_init"].reshape(N, T // L, L)[:, :, 1:].any() and rk["actor_rnn_state"].abs().max() > 0
        params = ({k: v.detach().clone() for k, v in actor.names().items()}, {k: v.detach().clone() for k, v in critic.names().items()})
        _ROLLOUTS[(N, T)] = (params, {k: _to(v, "cuda") for k, v in kw.items()}, {k: _to(v, "cuda") for k, v in rk.items()})
    return _ROLLOUTS[(N, T)]


def _learner(params, seed):
    actor, critic = ({k: v.clone().cuda() for k, v in p.items()} for p in params)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return learner.RecurrentDeviceLearner(actor, critic, CFG, tp_net=U.predictor(3, 41).cuda(), value_normalizer=learner.ValueNorm1().cuda(), generator=gen)


def _snapshot(lrn):
    """Parameters of the three networks, the three Adam states, ValueNorm1."""
    out = [v.detach().clone() for v in (*lrn.actor.values(), *lrn.critic.values(), *tp_train.parameters(lrn.tp_net))]
    assert lrn.tp_opt.state_dict()["state"]
    for opt in (lrn.actor_opt, lrn.critic_opt, lrn.tp_opt):
        for st in opt.state_dict()["state"].values():
            out += [st["step"].clone().cuda(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    vn = lrn.value_normalizer
    return out + [vn.running_mean.clone(), vn.running_mean_sq.clone(), vn.debiasing_term.clone()]


def _by_hand(lrn, kw, rk):
    """train_rollout's blocks through the public calls, every workspace allocated by the call that needs it."""
    xs, xo, xc = kw["obs_self"], kw["obs_others"], kw["obs_cylinders"]
    N, T = kw["reward"].shape[:2]
    nv = lrn.policy.forward(*kw["next_obs_last"], critic_state=rk["last_critic_rnn_state"], is_init=rk["last_is_init"], value_only=True).value
    adv, ret, _, (am, asd) = gae.rollout_targets(kw["reward"], kw["done"].unsqueeze(-1), kw["state_value"], nv, lrn.gamma, lrn.gae_lambda,
                                                 value_normalizer=lrn.value_normalizer, normalize_advantages=True, return_moments=True)
    M = lrn.num_minibatches
    tp_loss = tp_train.update_tp(lrn.tp_net, *kw["tp"], U.FUTURE, 1, M, lrn.tp_epochs, lrn.tp_opt, generator=lrn.generator)   # draws first
    table = torch.empty(lrn.ppo_epochs * M, len(learner.COLUMNS), device="cuda")
    m = 0
    for _ in range(lrn.ppo_epochs):
        perm = torch.randperm((N * (T // L) // M) * M, device="cuda", generator=lrn.generator).reshape(M, -1)
        for idx in perm:
            rnn_train.update_actor_rnn(lrn.actor, xs, xo, xc, rk["actor_rnn_state"], rk["is_init"], kw["action"], kw["log_probs"], adv, lrn.actor_opt,
                                       segment=idx, cfg=lrn.cfg, out=table[m, :4])
            rnn_train.update_critic_rnn(lrn.critic, xs, xo, xc, rk["critic_rnn_state"], rk["is_init"], kw["state_value"], ret, lrn.critic_opt,
                                        segment=idx, cfg=lrn.cfg, out=table[m, 4:])
            m += 1
    head = lrn._info_row(kw["action"], table).tolist()
    info = dict(zip(learner.COLUMNS + ("action_norm",), head))
    info["TP_loss"], info["advantages_mean"], info["advantages_std"] = float(tp_loss), float(am), float(asd)
    info["value_running_mean"] = float(lrn.value_normalizer.running_mean.mean())
    return {f"drone/{k}": info[k] for k in learner.INFO_KEYS if k in info}


def _guard_the_loop(lrn):
    """The PPO loop under set_sync_debug_mode("error"): a host synchronisation inside it raises."""
    loop = lrn._ppo_loop

    def guarded(*a, **k):
        torch.cuda.set_sync_debug_mode("error")
        try:
            return loop(*a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    lrn._ppo_loop = guarded


@pytest.mark.parametrize("N,T", [(8, 32), (5, 16)])
def test_train_rollout_equals_the_hand_driven_calls_bit_for_bit(N, T):
    params, kw, rk = _rollout(N, T)
    assert (N * (T // L)) % 2 == (0 if N == 8 else 1)             # [5, 16]: five segments, two minibatches of two, one dropped
    a, b = _learner(params, 7), _learner(params, 7)
    _guard_the_loop(a)
    ia = a.train_rollout(**kw, **rk)
    ib = _by_hand(b, kw, rk)
    assert list(ia) == list(ib) == [f"drone/{k}" for k in learner.INFO_KEYS]
    for k in ia:
        assert np.float32(ia[k]) == np.float32(ib[k]) and np.isfinite(ia[k]), (k, ia[k], ib[k])
    sa, sb = _snapshot(a), _snapshot(b)
    assert len(sa) == len(sb) and all(torch.equal(x, y) for x, y in zip(sa, sb))
    assert not torch.equal(next(iter(a.actor.values())), params[0][next(iter(params[0]))].cuda())      # the parameters moved


def test_a_learner_whose_workspaces_regrow_equals_a_fresh_one():
    small, big = _rollout(5, 16), _rollout(8, 32)
    a = _learner(big[0], 3)
    sd = copy.deepcopy(a.state_dict())
    assert "TP" in sd and "TP_opt" in sd
    a.train_rollout(**small[1], **small[2])                       # workspaces sized for two segments a minibatch
    a.load_state_dict(sd)
    a.generator = torch.Generator(device="cuda").manual_seed(11)
    b = _learner(big[0], 3)
    b.load_state_dict(copy.deepcopy(sd))
    b.generator = torch.Generator(device="cuda").manual_seed(11)
    ia, ib = a.train_rollout(**big[1], **big[2]), b.train_rollout(**big[1], **big[2])    # ... regrown for eight
    assert ia == ib
    assert all(torch.equal(x, y) for x, y in zip(_snapshot(a), _snapshot(b)))


def test_the_recurrent_example_trains_through_the_learner():
    script = os.path.join(ROOT, "examples", "recurrent_policy.py")
    run = subprocess.run([sys.executable, script, "--envs", "64", "--steps", "16", "--updates", "1", "--learner"], capture_output=True, text=True,
                         timeout=240)
    assert run.returncode == 0, run.stdout + run.stderr
    for it in (0, 1):
        line = next(ln for ln in run.stdout.splitlines() if ln.startswith(f"rollout {it}: "))
        for k in learner.INFO_KEYS:                            # TP_loss among them: the env's predictor trains beside the networks
            assert f"{k} " in line, (k, line)
