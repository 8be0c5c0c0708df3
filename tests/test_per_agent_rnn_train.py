"""The recurrent update with one actor per agent on the CPU (hns_amd.rnn_train.policy_loss_and_grad_rnn_per_agent /
update_actor_rnn_per_agent, learner.PerAgentRecurrentDeviceLearner).  The device kernels:
tests/test_hip_per_agent_rnn_train.py; the cases, the independent per-agent flow and the planted defects: tests/per_agent_rnn_update_cases.py.

  * the statements: the CPU path's flow (rnn_train._torch_forward / _torch_update with the stacked head's restatement) run in fp64 against fp64
    autograd of the reference's statements written independently — one module set per agent, the loss over all rows — to 1e-10 of the largest
    entry; and the public call in fp32 within the gate, per stacked tensor and per agent slice;
  * the loss and entropy rules; A = 1 against policy_loss_and_grad_rnn on slice 0;
  * PerAgentRecurrentDeviceLearner: one train_rollout on CPU tensors equals the hand-driven calls bit for bit; state_dict round trip; refusals;
  * the three size queries against the plan restated from the kernels' constants, and 0 for the invalid shapes; each case's reach;
  * the gate's teeth: one planted plan-limited defect per padded structure, rejected."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import per_agent_rnn_update_cases as PC
import rnn_update_reference as U
from hns_amd import abi, gae, learner, rnn_train
from hns_amd import policy as P
from hns_amd import policy_train as PT
from hns_amd import rnn as RN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hns_encoder_agents_workspace_bytes", "hns_encoder_forward_agents", "hns_encoder_backward_agents", "hns_gru_agents_workspace_bytes",
       "hns_gru_forward_agents", "hns_gru_backward_agents", "hns_rnn_actor_head_agents_workspace_bytes", "hns_rnn_actor_head_grad_agents")
TOL = 1e-10
SMALL = PC.Case(3, 5, 35, 3, 8, 4, 5)
_t = lambda v: torch.as_tensor(np.asarray(v)).clone()            # noqa: E731


def _names():
    """{reference name: (group, field)} of rnn_train.network_parameters' three mappings for the actor."""
    out = {k: ("encoder" if f not in ("head_w", "head_b", "log_std") else "head", f) for k, f in P.ACTOR_NAMES.items()}
    out.update({"rnn." + k: ("gru", f) for k, f in RN.NAMES.items()})
    return out


@pytest.fixture(scope="module")
def small():
    return PC.build(SMALL, 903, seg=[4, 0, 5, 2, 1])


def test_the_cpu_paths_statements_in_fp64_equal_fp64_autograd_of_the_references_statements(small):
    b = small
    A, K, D, N, T, L, B = b.case
    net32 = rnn_train.network_parameters({k: _t(v) for k, v in b.net.items()}, True, stacked=True)
    net = rnn_train.Network(*({f: t.double() for f, t in grp.items()} for grp in net32))
    xs, xo, xc = PT.as_rollout(*(_t(b.obs[k]).double() for k in ("state_self", "state_others", "cylinders")))
    seg = _t(b.seg)
    per_row = [(_t(r).double(), w) for r, w in zip(b.rows, (4, 1, 1))]
    fwd = rnn_train._torch_forward(net, xs, xo, xc, (N, T, A, D, K), seg, L, N * (T // L), _t(b.state).double(), _t(b.is_init), per_row)
    res = rnn_train._torch_update(net, fwd, lambda p, y, a, lpo, adv: rnn_train.actor_head(p["head_w"], p["head_b"], p["log_std"], y, a, lpo, adv, 0.1, 1e-3))
    names = _names()
    assert set(names) == set(b.net)
    got = {k: getattr(net, grp)[f].grad.numpy() for k, (grp, f) in names.items()}
    got.update({k: res[k].numpy() for k in ("policy_loss", "entropy", "ess", "log_probs")})
    for k, g in got.items():
        want = b.g64[k] if k in b.g64 else b.s64[k]
        assert g.shape == want.shape, k
        assert np.abs(g - want).max() <= TOL * max(np.abs(want).max(), 1e-300), (k, np.abs(g - want).max(), np.abs(want).max())


def test_the_public_call_in_fp32_against_the_independent_per_agent_flow(small):
    b = small
    assert not PC.preconditions(b)
    assert b.is_init[0, 0, 0] and b.is_init[b.case.N - 1, b.case.L // 2, 0] and np.abs(b.state).min() > 0
    live, res = PC.call(b, _t)
    assert all(v.grad.shape == v.shape and v.dim() >= 2 and v.shape[0] == b.case.A for v in live.values())
    worst, bad = U.gate("small", PC.items(b, PC.outputs(b, live, res)))
    assert not bad, "; ".join(bad)
    with pytest.raises(NotImplementedError):
        PC.call(b, _t, global_rows=b.case.B * b.case.L * b.case.A)
    with pytest.raises(NotImplementedError):
        PC.call(b, _t, group="world")


def test_the_loss_and_entropy_rules(small):
    b = small
    A = b.case.A
    live, res = PC.call(b, _t)
    # policy_loss: the mean over ALL rows = the mean over the agents of the per-agent means (every agent has B L rows)
    ref = float(b.s64["agent_loss"].mean())
    assert abs(float(b.s64["policy_loss"]) - ref) <= 1e-14 * abs(ref)
    assert abs(float(res.policy_loss) - ref) <= 8 * max(abs(float(b.s32["policy_loss"]) - ref), 2.0 ** -24 * abs(ref))
    # entropy: the mean over the agents of each agent's (the agents' log_std differ)
    assert np.ptp(b.s64["agent_entropy"]) > 0.1
    assert abs(float(res.entropy) - float(b.s64["agent_entropy"].mean())) <= 8 * 2.0 ** -24 * abs(float(res.entropy))
    # each agent's d log_std holds -entropy_coef / A exactly once: the restatement in fp64 at two coefficients
    y = torch.randn(2, 3, A, 128, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    hw, hb, ls = (live[k].double() for k in ("act_dist.fc_mean.weight", "act_dist.fc_mean.bias", "act_dist.log_std"))
    g = torch.Generator().manual_seed(2)
    act, lpo, adv = torch.randn(2, 3, A, 4, dtype=torch.float64, generator=g), torch.randn(2, 3, A, dtype=torch.float64, generator=g) - 6, \
        torch.randn(2, 3, A, dtype=torch.float64, generator=g)
    r0, r1 = (rnn_train.actor_head(hw, hb, ls, y, act, lpo, adv, 0.1, ec) for ec in (0.0, 0.3))
    assert tuple(r1["d_log_std"].shape) == (A, 4) and tuple(r1["d_head_w"].shape) == (A, 4, 128)
    assert (r1["d_log_std"] - r0["d_log_std"] + 0.3 / A).abs().max() <= 1e-15
    for k in ("dy", "d_head_w", "d_head_b", "policy_loss", "entropy", "ess", "log_probs"):
        assert torch.equal(r0[k], r1[k]), k
    # ... and through the whole call in fp32
    live0 = {k: _t(v) for k, v in b.net.items()}
    res0 = rnn_train.policy_loss_and_grad_rnn_per_agent(live0, _t(b.obs["state_self"]), _t(b.obs["state_others"]), _t(b.obs["cylinders"]), _t(b.state),
                                                        _t(b.is_init), *(_t(r) for r in b.rows), segment=_t(b.seg), seq_len=b.case.L, entropy_coef=0.0)
    d = live["act_dist.log_std"].grad - live0["act_dist.log_std"].grad
    assert (d + 1e-3 / A).abs().max() <= 2.0 ** -23 * live0["act_dist.log_std"].grad.abs().max() and torch.equal(res0.log_probs, res.log_probs)


def test_one_stacked_agent_equals_the_shared_update_on_slice_0():
    """A = 1: every result within the gate's bound with the shared call in the fp32 reference's place — e(stacked) <= 8 max(e(shared),
    2^-24 max|ref_64|) against the fp64 flow — which is equality up to fp32 rounding (the stacked head sums by einsum)."""
    case = PC.Case(1, 5, 20, 3, 8, 4, 5)
    b = PC.build(case, 901, seg=[4, 0, 5, 2, 1])
    live, res = PC.call(b, _t)
    shared = {k: _t(v[0]) for k, v in b.net.items()}
    ref = rnn_train.policy_loss_and_grad_rnn(shared, _t(b.obs["state_self"]), None, _t(b.obs["cylinders"]), _t(b.state), _t(b.is_init),
                                            *(_t(r) for r in b.rows), segment=_t(b.seg), seq_len=case.L, entropy_coef=1e-3)
    its = [(k, live[k].grad.numpy()[0], b.g64[k][0], shared[k].grad.numpy()) for k in b.net]
    its += [(k, getattr(res, k).numpy(), b.s64[k], getattr(ref, k).numpy()) for k in ("policy_loss", "entropy", "ess", "grad_norm")]
    its.append(("log_probs", res.log_probs.squeeze(-1).numpy(), b.s64["log_probs"], ref.log_probs.squeeze(-1).numpy()))
    worst, bad = U.gate("A=1", its)
    assert not bad, "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------- the learner
def _learner(actor, critic, seed):
    a, c = ({k: v.clone() for k, v in p.items()} for p in (actor, critic))
    return learner.PerAgentRecurrentDeviceLearner(a, c, {**PC.LEARNER_CFG, "ppo_epochs": 2, "actor": {"rnn": {"train_seq_len": 4}},
                                                         "critic": {"rnn": {"train_seq_len": 4}}}, value_normalizer=learner.ValueNorm1(),
                                                  generator=torch.Generator().manual_seed(seed))


def _snapshot(lrn):
    out = [v.detach().clone() for v in (*lrn.actor.values(), *lrn.critic.values())]
    for opt in (lrn.actor_opt, lrn.critic_opt):
        for st in opt.state_dict()["state"].values():
            out += [st["step"].clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    vn = lrn.value_normalizer
    return out + [vn.running_mean.clone(), vn.running_mean_sq.clone(), vn.debiasing_term.clone()]


def _by_hand(lrn, kw, rk):
    xs, xo, xc = kw["obs_self"], kw["obs_others"], kw["obs_cylinders"]
    N, T = kw["reward"].shape[:2]
    L, M = lrn.train_seq_len, lrn.num_minibatches
    nv = lrn.policy.forward(*kw["next_obs_last"], critic_state=rk["last_critic_rnn_state"], is_init=rk["last_is_init"], value_only=True).value
    adv, ret, _, (am, asd) = gae.rollout_targets(kw["reward"], kw["done"].unsqueeze(-1), kw["state_value"], nv, lrn.gamma, lrn.gae_lambda,
                                                 value_normalizer=lrn.value_normalizer, normalize_advantages=True, return_moments=True)
    rows = []
    for _ in range(lrn.ppo_epochs):
        for idx in torch.randperm((N * (T // L) // M) * M, generator=lrn.generator).reshape(M, -1):
            sa = rnn_train.update_actor_rnn_per_agent(lrn.actor, xs, xo, xc, rk["actor_rnn_state"], rk["is_init"], kw["action"], kw["log_probs"], adv,
                                                      lrn.actor_opt, segment=idx, cfg=lrn.cfg)
            sc = rnn_train.update_critic_rnn(lrn.critic, xs, xo, xc, rk["critic_rnn_state"], rk["is_init"], kw["state_value"], ret, lrn.critic_opt,
                                             segment=idx, cfg=lrn.cfg)
            rows.append(torch.stack([(sa | sc)[k].reshape(()).float() for k in learner.COLUMNS]))
    a = kw["action"].reshape(-1, 4).double()
    info = dict(zip(learner.COLUMNS, learner._mean_row(torch.stack(rows))))
    info["action_norm"] = float(np.float32(a.square().sum(-1).sqrt().sum().item() / a.shape[0]))
    info["advantages_mean"], info["advantages_std"] = float(am), float(asd)
    info["value_running_mean"] = float(lrn.value_normalizer.running_mean.mean())
    return {f"drone/{k}": info[k] for k in learner.INFO_KEYS if k in info}


@pytest.fixture(scope="module")
def rollout():
    actor, critic, kw, rk = PC.learner_rollout(PC.Case(3, 5, 35, 5, 8, 4, 5), 905)
    return actor, critic, kw, rk


def test_train_rollout_equals_the_hand_driven_calls_bit_for_bit(rollout):
    actor, critic, kw, rk = rollout
    a, b = _learner(actor, critic, 5), _learner(actor, critic, 5)
    assert isinstance(a, learner.RecurrentDeviceLearner) and isinstance(a.policy, P.PerAgentRecurrentDevicePolicy) and a.train_seq_len == 4
    assert len(a._network_tensors()[0]) == 29 and all(t.shape[0] == 3 for t in a._network_tensors()[0])
    ia, ib = a.train_rollout(**kw, **rk), _by_hand(b, kw, rk)
    assert list(ia) == list(ib)
    for k in ia:
        assert np.float32(ia[k]) == np.float32(ib[k]) and np.isfinite(ia[k]), (k, ia[k], ib[k])
    sa, sb = _snapshot(a), _snapshot(b)
    assert len(sa) == len(sb) and all(torch.equal(x, y) for x, y in zip(sa, sb))
    for k, v in actor.items():
        for ag in range(3):
            assert not torch.equal(a.actor[k][ag], v[ag]), (k, ag)


def test_state_dict_round_trips_into_a_fresh_learner_that_takes_an_identical_step(rollout):
    actor, critic, kw, rk = rollout
    lrn = _learner(actor, critic, 1)
    lrn.train_rollout(**kw, **rk)
    sd = copy.deepcopy(lrn.state_dict())
    assert sd["actor_params"]["rnn.cell.weight_ih"].shape == (3, 384, 128) and sd["critic"]["rnn.cell.weight_ih"].shape == (384, 128)
    fresh = _learner({k: torch.randn_like(v) * 0.05 for k, v in actor.items()}, {k: torch.randn_like(v) * 0.05 for k, v in critic.items()}, 2)
    fresh.load_state_dict(sd)
    lrn.generator, fresh.generator = torch.Generator().manual_seed(2), torch.Generator().manual_seed(2)
    assert lrn.train_rollout(**kw, **rk) == fresh.train_rollout(**kw, **rk)
    assert all(torch.equal(x, y) for x, y in zip(_snapshot(lrn), _snapshot(fresh)))


def test_refusals(rollout):
    actor, critic, kw, rk = rollout
    cfg = PC.LEARNER_CFG
    mk = learner.PerAgentRecurrentDeviceLearner
    with pytest.raises(NotImplementedError, match="group"):
        mk(actor, critic, cfg, group="world")
    shared = {k: v[0] for k, v in actor.items()}
    with pytest.raises(P.PolicyConfigError, match="leading agent dimension"):           # actor tensors that are not stacked
        mk(shared, critic, cfg)
    with pytest.raises(P.PolicyConfigError, match="share_actor"):
        mk(actor, critic, {**cfg, "share_actor": True})
    plain_c = {k: v for k, v in critic.items() if not k.startswith("rnn.")}
    plain_a = {k: v for k, v in actor.items() if not k.startswith("rnn.")}
    for pol in (P.RecurrentDevicePolicy(shared, critic), P.PerAgentDevicePolicy(plain_a, plain_c), P.DevicePolicy({k: v[0] for k, v in plain_a.items()}, plain_c)):
        with pytest.raises(P.PolicyConfigError, match="PerAgentRecurrentDevicePolicy"):  # a policy that is not both per-agent and recurrent
            mk(actor, critic, cfg, device_policy=pol)
    with pytest.raises(P.PolicyConfigError):                                             # no GRU in the stacked actor
        mk(plain_a, critic, cfg)
    with pytest.raises(P.PolicyConfigError):                                             # a stacked critic
        mk(actor, {k: torch.stack([v, v]) for k, v in critic.items()}, cfg)
    # the four existing learners keep refusing the configuration; the recurrent ones name the open item
    pol = P.PerAgentRecurrentDevicePolicy(actor, critic)
    rcfg = {"actor": {"rnn": {"cls": "gru"}}, "critic": {"rnn": {"cls": "gru"}}}
    with pytest.raises(P.PolicyConfigError, match="open item"):
        learner.RecurrentDeviceLearner(actor, critic, rcfg)
    with pytest.raises(P.PolicyConfigError, match="open item"):
        learner.DataParallelRecurrentLearner(shared, critic, rcfg, group="world", device_policy=pol)
    with pytest.raises(P.PolicyConfigError, match="recurrent"):
        learner.PerAgentDeviceLearner(plain_a, plain_c, {"share_actor": False}, device_policy=pol)
    with pytest.raises(P.PolicyConfigError, match="recurrent"):
        learner.DeviceLearner(None, None, {}, device_policy=pol)
    # the functions
    args = (kw["obs_self"], kw["obs_others"], kw["obs_cylinders"], rk["actor_rnn_state"], rk["is_init"], kw["action"], kw["log_probs"], kw["state_value"])
    opt = rnn_train.make_optimizer_per_agent(actor, {"share_actor": False})
    for extra in ({"global_rows": 60}, {"group": "world"}):
        with pytest.raises(NotImplementedError):
            rnn_train.update_actor_rnn_per_agent(actor, *args, opt, seq_len=4, **extra)
    with pytest.raises(TypeError, match="ClippedAdam"):
        rnn_train.update_actor_rnn_per_agent(actor, *args, torch.optim.Adam(list(actor.values())), seq_len=4)
    with pytest.raises(P.PolicyConfigError):
        rnn_train.make_optimizer_per_agent(actor, {"share_actor": True})
    with pytest.raises(P.PolicyConfigError):
        rnn_train.policy_loss_and_grad_rnn_per_agent(shared, *args, seq_len=4)
    with pytest.raises(ValueError, match="agents"):                                      # the observation's agents against the stacked actor's
        rnn_train.policy_loss_and_grad_rnn_per_agent({k: v[:2].contiguous() for k, v in actor.items()}, *args, seq_len=4)
    with pytest.raises(IndexError):
        rnn_train.policy_loss_and_grad_rnn_per_agent(actor, *args, segment=torch.tensor([0, 10]), seq_len=4)


# ---------------------------------------------------------------------------------------------------------------- plans, sizes, reach
@pytest.mark.parametrize("tag", PC.TAGS)
def test_each_case_reaches_what_it_is_there_for_and_the_size_queries_equal_the_restated_plan(tag):
    c = PC.CASES[tag]
    p = PC.plan(c)
    assert PC.REACH[tag](p, c), (tag, p)
    A, K, D, N, T, L, B = c
    assert B < p["segments"] and (B == 1 or 0 in PC.C.minibatch(c, PC.SEEDS[tag] + 2000)) and PC.C.flagged_segment(c) in PC.C.minibatch(c, PC.SEEDS[tag] + 2000)
    lib = abi.load_library()
    assert lib.hns_gru_agents_workspace_bytes(B, A, L, 1) == p["gru_bytes"] and lib.hns_gru_agents_workspace_bytes(B, A, L, 0) == 0
    assert lib.hns_encoder_agents_workspace_bytes(p["rows"], D, A, K, 1) == p["enc_bytes"]
    assert lib.hns_encoder_agents_workspace_bytes(p["rows"], D, A, K, 0) == p["enc_forward_bytes"]
    assert lib.hns_rnn_actor_head_agents_workspace_bytes(B, A, L) == p["head_bytes"]
    for d in PC.DEFECTS:                                         # the structure every planted defect needs exists at every case it is planted at
        assert (tag in PC.DEFECT_TABLE[d]) <= bool(PC.defect_keep(d, c)), (d, tag)


def test_the_size_queries_return_0_for_invalid_shapes_and_the_abi_declares_the_entries():
    lib = abi.load_library()
    raw = ctypes.CDLL(abi.library_path())
    header = open(os.path.join(ROOT, "include", "hns.h")).read()
    for sym in NEW:
        getattr(raw, sym)
        assert sym in abi.EXPORTED_SYMBOLS and sym + "(" in header, sym
    assert lib.hns_abi_version() == 8                            # purely additive
    for shape in ((0, 3, 16, 1), (5, 0, 16, 1), (5, 8, 16, 1), (5, 3, 0, 1), (5, 3, 65, 1), (2 ** 40, 3, 16, 1)):
        assert lib.hns_gru_agents_workspace_bytes(*shape) == 0, shape
    assert lib.hns_gru_agents_workspace_bytes(5, 7, 64, 1) > 0
    for shape in ((0, 35, 3, 5, 1), (100, 35, 3, 5, 1), (96, 0, 3, 5, 1), (96, abi.HNS_POLICY_MAX_SELF_DIM + 1, 3, 5, 1), (96, 35, 0, 5, 1), (96, 35, 8, 5, 1), (96, 35, 3, 0, 1),
                  (96, 35, 3, 17, 1), (2, 35, 3, 5, 0)):            # (100 and 2 rows: no multiple of 3 agents)
        assert lib.hns_encoder_agents_workspace_bytes(*shape) == 0, shape
    assert lib.hns_encoder_agents_workspace_bytes(96, 35, 3, 5, 0) > 0
    for shape in ((0, 3, 16), (1, 0, 16), (1, 8, 16), (1, 3, 0), (1, 3, 65), (2 ** 40, 3, 16)):
        assert lib.hns_rnn_actor_head_agents_workspace_bytes(*shape) == 0, shape
    assert lib.hns_rnn_actor_head_agents_workspace_bytes(1, 3, 1) >= 3 * 528 * 8
    # the entries refuse bad arguments before any launch, without a device
    net, seq = abi.HnsGruNet(), abi.HnsGruSeq()
    assert lib.hns_gru_forward_agents(ctypes.byref(net), ctypes.byref(seq), None, None, None, None, 0, None) != abi.HNS_OK
    assert b"aligned" in lib.hns_last_error() or b"NULL" in lib.hns_last_error()
    assert lib.hns_rnn_actor_head_grad_agents(*([None] * 4), None, None, None, 0.1, 0.0, *([None] * 9), 0, None) != abi.HNS_OK
    assert lib.hns_encoder_forward_agents(None, None, 35, 3, 5, None, None, 0, None) != abi.HNS_OK


# ---------------------------------------------------------------------------------------------------------------- the gate's teeth
@pytest.mark.parametrize("defect,tag", [(d, t) for d in PC.DEFECTS for t in PC.DEFECT_TABLE[d]])
def test_the_gate_rejects_each_planted_defect(defect, tag):
    b = PC.refs(tag)
    assert not PC.preconditions(b)
    g, s = PC.defect_flow(b, defect)
    worst, bad = U.gate(f"{defect}@{tag}", PC.items(b, {**g, **s}), verbose=False)
    assert bad and worst > U.BAR, (defect, tag, worst)
    sound, ok = U.gate(tag, PC.items(b, {**b.g32, **b.s32}), verbose=False)            # (the fp32 flow itself passes at ratio <= 1)
    assert not ok and sound <= 1.0
