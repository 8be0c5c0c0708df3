"""hns_amd.learner.DeviceLearner on the CPU: MAPPOPolicy.train_op (learning/mappo.py:363-475) as ONE call against the same blocks driven by
hand through the package's public functions (tests/learner_cases.py) — bit for bit: every parameter, every Adam moment and step counter,
ValueNorm1's buffers, every info value — and the order in which the index rows are drawn and used (the predictor's epochs first; per
minibatch the actor, then the critic).  Also: the dropped remainder of make_dataset_naive, every refused configuration, the checkpoint
round trip, a reference checkpoint without optimisers, the "critic" / "TP" entries in plain torch.nn modules, hns_learner_info's refusals
through ctypes (no GPU needed), the info keys."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import learner_cases as LC
from hns_amd import abi, learner
from hns_amd import policy as P

N, T, A = 6, 8, 3


@pytest.fixture(scope="module")
def start():
    state = LC.make_state(A, 11)
    return state, LC.make_rollout(state, N, T, A, 12)


def _record(monkeypatch):
    """Records ("tp" | "actor" | "critic", index row) at the three update entry points the learner goes through."""
    events = []
    real_tp, real_a, real_c = learner.tp_train.loss_and_grad, learner.actor_train.update_actor, learner.critic_train.update_critic

    def tp(tpn, x, y, index=None, **kw):
        events.append(("tp", index.tolist()))
        return real_tp(tpn, x, y, index, **kw)

    def actor(*a, index=None, **kw):
        events.append(("actor", index.tolist()))
        return real_a(*a, index=index, **kw)

    def critic(*a, index=None, **kw):
        events.append(("critic", index.tolist()))
        return real_c(*a, index=index, **kw)

    monkeypatch.setattr(learner.tp_train, "loss_and_grad", tp)
    monkeypatch.setattr(learner.actor_train, "update_actor", actor)
    monkeypatch.setattr(learner.critic_train, "update_critic", critic)
    return events


def _check_info(info, hand, use_tp=True):
    for k in learner.COLUMNS + ("advantages_mean", "advantages_std", "value_running_mean") + (("TP_loss",) if use_tp else ()):
        assert np.float32(info[f"drone/{k}"]).tobytes() == np.float32(hand[k]).tobytes(), (k, info[f"drone/{k}"], hand[k])
    # the CPU path forms action_norm as the kernel does: fp64 throughout, rounded once
    assert np.float32(info["drone/action_norm"]).tobytes() == np.float32(hand["action_norm_f64"]).tobytes()


def test_train_op_is_the_hand_driven_sequence_bit_for_bit(start, monkeypatch):
    state0, ro = start
    hand_state = LC.clone_state(state0)
    opts = LC.hand_optimisers(hand_state)
    trace = []
    hand = LC.hand_train_op(hand_state, opts, ro, torch.Generator().manual_seed(5), trace=trace)

    state = LC.clone_state(state0)
    L = LC.make_learner(state, seed=5)
    events = _record(monkeypatch)
    info = L.train_op(LC.as_tensordict(ro))
    assert L.n_updates == 1
    LC.assert_same_state(LC.state_tensors(state, LC.learner_opts(L)), LC.state_tensors(hand_state, opts), "train_op against the hand sequence")
    _check_info(info, hand)
    # the order: the predictor's TP_epochs x 4 rows first (one RNG stream, they draw first), then per PPO minibatch the actor and then the
    # critic on the SAME row
    want = [e for e in trace if e[0] == "tp"]
    for _, row in (e for e in trace if e[0] == "ppo"):
        want += [("actor", row), ("critic", row)]
    assert len(want) == 4 + 2 * 2 * 4
    assert events == want
    assert all(len(row) == N * T // 4 for kind, row in events if kind != "tp") and all(len(row) == N * (T - LC.FUTURE) // 4 for kind, row in events if kind == "tp")
    # a second call continues from the optimisers' state and the generator's: still the hand sequence
    hand2 = LC.hand_train_op(hand_state, opts, ro, torch.Generator().manual_seed(6))
    L.generator.manual_seed(6)
    info2 = L.train_rollout(**ro)
    LC.assert_same_state(LC.state_tensors(state, LC.learner_opts(L)), LC.state_tensors(hand_state, opts), "second call")
    _check_info(info2, hand2)
    assert L.n_updates == 2 and float(L.actor_opt.state[next(iter(state["actor"].values()))]["step"]) == 16.0


def test_the_remainder_of_make_dataset_naive_is_dropped(monkeypatch):
    """N T = 35 env-steps in 4 minibatches: 8 each over a permutation of the first 32, the last 3 never visited (mappo.py:507-511)."""
    state = LC.make_state(A, 21)
    ro = LC.make_rollout(state, 5, 7, A, 22)
    L = LC.make_learner(state, seed=1, use_tp=False)
    events = _record(monkeypatch)
    L.train_rollout(**ro)
    for kind in ("actor", "critic"):
        rows = [row for k, row in events if k == kind]
        assert len(rows) == 2 * 4 and all(len(r) == 8 for r in rows)
        visits = np.bincount(np.concatenate(rows), minlength=35)
        assert visits[:32].tolist() == [2] * 32 and visits[32:].tolist() == [0, 0, 0]
    assert not [e for e in events if e[0] == "tp"]


class _Untouchable:
    """Stands for the networks in a refused construction: any use raises."""

    def __getattr__(self, name):
        raise AssertionError(f"the refused learner touched its network ({name})")


@pytest.mark.parametrize("patch, exc", [
    ({"share_actor": False}, P.PolicyConfigError), ({"critic_input": "state"}, P.PolicyConfigError),
    ({"actor": {"rnn": {"cls": "gru"}}}, P.PolicyConfigError), ({"critic": {"rnn": {"cls": "gru"}}}, P.PolicyConfigError),
    ({"actor": {"tanh": True}}, P.PolicyConfigError), ({"actor": {"lr_scheduler": "StepLR"}}, P.PolicyConfigError),
    ({"critic": {"lr_scheduler": "StepLR"}}, P.PolicyConfigError), ({"actor": {"weight_decay": 0.01}}, NotImplementedError),
    ({"critic": {"weight_decay": 0.01}}, NotImplementedError)])
def test_refused_configurations_raise_before_anything_is_built(patch, exc):
    cfg = copy.deepcopy(LC.CFG)
    for k, v in patch.items():
        if isinstance(v, dict):
            cfg[k].update(v)
        else:
            cfg[k] = v
    with pytest.raises(exc):
        learner.DeviceLearner(_Untouchable(), _Untouchable(), cfg, tp_net=_Untouchable())

    class Obj:                                                   # the same cfg as an attribute object
        def __init__(self, d):
            for k, v in d.items():
                setattr(self, k, Obj(v) if isinstance(v, dict) else v)
    with pytest.raises(exc):
        learner.DeviceLearner(_Untouchable(), _Untouchable(), Obj(cfg), tp_net=_Untouchable())


def test_state_dict_round_trips_bit_for_bit_with_the_optimisers(start):
    state0, ro = start
    a = LC.clone_state(state0)
    La = LC.make_learner(a, seed=3)
    La.train_rollout(**ro)
    sd = copy.deepcopy(La.state_dict())
    assert set(sd) == {"TP", "critic", "actor_params", "value_normalizer", "actor_opt", "critic_opt", "TP_opt"}
    assert set(sd["actor_opt"]) == {"state", "param_groups"} and set(sd["actor_opt"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    torch.optim.Adam(list(a["actor"].values()), lr=5e-4).load_state_dict(sd["actor_opt"])           # torch.optim.Adam's format
    b = LC.make_state(A, 99)                                     # another initialisation altogether
    Lb = LC.make_learner(b, seed=0)
    versions = [p._version for p in (*b["actor"].values(), *b["critic"].parameters(), *b["tp"].parameters())]
    Lb.load_state_dict(sd)
    assert all(p._version > v for p, v in zip((*b["actor"].values(), *b["critic"].parameters(), *b["tp"].parameters()), versions))
    LC.assert_same_state(LC.state_tensors(b, LC.learner_opts(Lb)), LC.state_tensors(a, LC.learner_opts(La)), "after load_state_dict")
    La.generator.manual_seed(8)
    Lb.generator.manual_seed(8)
    ia, ib = La.train_rollout(**ro), Lb.train_rollout(**ro)
    assert ia == ib
    LC.assert_same_state(LC.state_tensors(b, LC.learner_opts(Lb)), LC.state_tensors(a, LC.learner_opts(La)), "one train_op after the load")


def test_a_reference_checkpoint_without_optimiser_keys_loads_with_fresh_optimisers(start):
    state0, ro = start
    a = LC.clone_state(state0)
    La = LC.make_learner(a, seed=3)
    La.train_rollout(**ro)
    sd = {k: v for k, v in copy.deepcopy(La.state_dict()).items() if not k.endswith("_opt")}
    assert set(sd) == {"TP", "critic", "actor_params", "value_normalizer"}                       # mappo.py:477-484
    b = LC.make_state(A, 98)
    Lb = LC.make_learner(b, seed=0)
    Lb.train_rollout(**ro)                                       # its optimisers hold moments that must not survive the load
    Lb.load_state_dict(sd)
    assert all(len(o.state) == 0 for o in (Lb.actor_opt, Lb.critic_opt, Lb.tp_opt))
    none = {"actor": None, "critic": None, "tp": None}
    LC.assert_same_state(LC.state_tensors(b, none), LC.state_tensors(a, none), "parameters and ValueNorm1 after the load")
    Lb.train_rollout(**ro)                                       # and it trains on from there
    assert float(Lb.critic_opt.state[next(iter(b["critic"].parameters()))]["step"]) == 8.0


def test_critic_and_tp_entries_load_into_plain_torch_modules(start):
    state0, ro = start
    L = LC.make_learner(LC.clone_state(state0), seed=3)
    L.train_rollout(**ro)
    sd = L.state_dict()
    critic = LC.PlainCritic(A)
    assert critic.load_state_dict(sd["critic"], strict=True)

    class TP(nn.Module):                                         # the reference's TP_net members (mappo.py:572-589)
        def __init__(self):
            super().__init__()
            self.lstm = nn.LSTM(7 + 3 * A, 64, 1, batch_first=True)
            self.fc = nn.Linear(64, 15)
    tp = TP()
    assert tp.load_state_dict(sd["TP"], strict=True)
    assert torch.equal(tp.fc.weight, L.tp_net.fc.weight) and torch.equal(critic.v_out.weight, dict(P._flatten(L.critic))["v_out.weight"])
    pol = P.DevicePolicy.from_checkpoint(sd)                     # and the forward pass reads the same checkpoint
    assert torch.equal(pol.critic_p["head_w"], critic.v_out.weight)


@pytest.mark.parametrize("use_tp", [True, False])
def test_info_keys_are_the_references(start, use_tp):
    state0, ro = start
    L = LC.make_learner(LC.clone_state(state0), seed=3, use_tp=use_tp)
    info = L.train_op(LC.as_tensordict(ro))
    want = {"policy_loss", "actor_grad_norm", "entropy", "ESS", "value_loss", "critic_grad_norm", "explained_var", "advantages_mean",
            "advantages_std", "action_norm", "value_running_mean"} | ({"TP_loss"} if use_tp else set())
    assert set(info) == {f"drone/{k}" for k in want}
    assert all(isinstance(v, float) and np.isfinite(v) for v in info.values())
    assert info["drone/advantages_std"] > 0                      # (of the advantages before the normalisation: the test below)


def test_advantage_moments_are_those_before_the_normalisation():
    g = torch.Generator().manual_seed(4)
    reward, value = torch.randn(4, 8, 3, 1, generator=g), torch.randn(4, 8, 3, 1, generator=g)
    done, nv = torch.rand(4, 8, 3, 1, generator=g) < 0.1, torch.randn(4, 3, 1, generator=g)
    raw, _, _ = LC.gae.rollout_targets(reward, done, value, nv, 0.99, 0.95, normalize_advantages=False)
    out = LC.gae.rollout_targets(reward, done, value, nv, 0.99, 0.95, return_moments=True)
    assert len(out) == 4 and len(LC.gae.rollout_targets(reward, done, value, nv, 0.99, 0.95)) == 3
    mean, std = out[3]
    assert mean.dtype == torch.float32 and mean.dim() == 0
    assert abs(float(mean) - float(raw.double().mean())) <= 2.0 ** -23 * max(1.0, abs(float(raw.double().mean())))
    assert abs(float(std) - float(raw.double().std())) <= 2.0 ** -22 * float(raw.double().std())    # torch.std: unbiased


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    lib = abi.load_library()
    lib.hns_last_error.restype = ctypes.c_char_p
    return lib


def test_learner_info_refuses_bad_arguments_before_any_launch(lib):
    """Every refusal happens on the host (no device needed): HNS_ERR_INVALID_ARG and a message naming the argument."""
    Pn = 4096                                                    # a non-NULL aligned address; nothing is launched for a refused call
    stride = (ctypes.c_int64 * 2)(4, 1)
    ok = dict(action=Pn, stride=stride, rows=192, act_dim=4, table=Pn, m=8, cols=7, out=Pn, ws=Pn, nbytes=256)

    def call(**kw):
        a = {**ok, **kw}
        return lib.hns_learner_info(a["action"], a["stride"], a["rows"], a["act_dim"], a["table"], a["m"], a["cols"], a["out"], a["ws"], a["nbytes"], None)

    for kw, msg in ((dict(action=None), b"null"), (dict(stride=None), b"null"), (dict(table=None), b"null"), (dict(out=None), b"null"),
                    (dict(ws=None), b"null"), (dict(action=Pn + 2), b"misaligned"), (dict(table=Pn + 1), b"misaligned"), (dict(out=Pn + 3), b"misaligned"),
                    (dict(ws=Pn + 4), b"misaligned"), (dict(rows=0), b"rows"), (dict(rows=-5), b"rows"), (dict(act_dim=0), b"act_dim"),
                    (dict(act_dim=9), b"act_dim"), (dict(m=0), b"minibatches"), (dict(cols=0), b"columns"), (dict(cols=17), b"columns"),
                    (dict(stride=(ctypes.c_int64 * 2)(-4, 1)), b"strides"), (dict(nbytes=0), b"workspace"), (dict(rows=2049, nbytes=8), b"workspace")):
        assert call(**kw) == abi.HNS_ERR_INVALID_ARG, kw
        assert msg in lib.hns_last_error(), (kw, lib.hns_last_error())
    assert lib.hns_learner_info_workspace_bytes(0) == 0 and lib.hns_learner_info_workspace_bytes(-1) == 0
    assert lib.hns_learner_info_workspace_bytes(1) == 256 and lib.hns_learner_info_workspace_bytes(2048) == 256
    assert lib.hns_learner_info_workspace_bytes(2048 * 32 + 1) == 512               # 33 workgroups' partials
    assert lib.hns_learner_info_workspace_bytes(1 << 40) == 8192                    # the grid is capped at 1 024 workgroups


def test_learner_kernels_have_no_spills_or_scratch(lib):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import kernel_resources
    ks = [k for k in kernel_resources.all_kernels(os.path.join(root, "build", "obj")) if k["object"] == "hns_learner.o"]
    names = {k["demangled"] for k in ks}
    assert {"hns_learner_norm_kernel<true>", "hns_learner_norm_kernel<false>", "hns_learner_info_kernel"} <= names, names
    for k in ks:
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
