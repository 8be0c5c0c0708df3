"""One actor per agent (share_actor: False), CPU part: the CPU paths of hns_amd.policy.PerAgentDevicePolicy, hns_amd.actor_train's *_per_agent
functions and hns_amd.learner.PerAgentDeviceLearner — against g_actor_per_agent.npz (the reference's update_actor with share_actor: False,
recorded) bit for bit, as test_actor_train.py holds the shared path to g_actor_update.npz; the forward against `torch_forward` with each
slice, exactly; parsing; every refusal before anything is built; the existing classes still refusing stacked parameters.  The device part is
tests/test_hip_per_agent.py."""
import copy
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

import actor_per_agent_reference as UA
import actor_update_reference as U
import learner_cases as LC
import per_agent_cases as PC
from hns_amd import abi, learner
from hns_amd import actor_train as AT
from hns_amd import encoder as ENC
from hns_amd import policy as P

BIG = 5


def _digest(arrs):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a, dtype=np.float32).tobytes() for a in arrs)).hexdigest()


def _npz(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("tag", ["a3k5d35", "a2k8d20"])
def test_cpu_update_matches_reference_golden_bit_for_bit(one_thread, tag):
    """The four scalars of both updates, every clipped gradient (in full or through the sha256 over all of them), the parameters after the
    two updates: the same bits as the reference's statements with share_actor: False, one Adam and one clip over the stacked tensors."""
    actors, obs, action, lpo, adv, index, ent_coef, rec = UA.golden_case(_npz("g_actor_per_agent"), _npz("g_policy"), tag)
    assert _digest(actors.values()) == str(rec["init_digest"])          # the tensors the generator started from
    A = obs["state_self"].shape[1]
    assert all(not np.array_equal(v[0], v[1]) for v in actors.values())  # genuinely different agents
    p = {k: torch.nn.Parameter(torch.as_tensor(v.copy())) for k, v in actors.items()}
    cfg = {"share_actor": False, "clip_param": 0.1, "entropy_coef": ent_coef, "max_grad_norm": 10.0, "actor": {"lr": 5e-4}}
    opt = AT.make_optimizer_per_agent(p, cfg)
    t = torch.as_tensor
    for u in (1, 2):
        st = AT.update_actor_per_agent(p, t(obs["state_self"]), t(obs["state_others"]), t(obs["cylinders"]), t(action), t(lpo), t(adv), opt,
                                       index=t(index), cfg=cfg, check_index=True)
        for mine, theirs in (("policy_loss", "policy_loss"), ("actor_grad_norm", "grad_norm"), ("entropy", "entropy"), ("ESS", "ESS")):
            assert np.float32(st[mine]) == rec[f"u{u}:{theirs}"], (u, mine, float(st[mine]), rec[f"u{u}:{theirs}"])
        grads = {k: v.grad.numpy() for k, v in p.items()}
        assert all(g.shape == v.shape and g.shape[0] == A for g, v in zip(grads.values(), p.values()))
        if u == 1:
            stored = [k for k in p if f"grad:{k}" in rec]
            assert len(stored) == len(p) - BIG
            for k in stored:
                assert np.array_equal(grads[k], rec[f"grad:{k}"]), k
        assert _digest(grads.values()) == str(rec[f"u{u}:grad_digest"]), u
    assert (float(rec["u1:grad_norm"]) > 10.0) == (tag == "a2k8d20")     # the case with the norm clip active
    for k, v in p.items():
        if f"final:{k}" in rec:
            assert np.array_equal(v.detach().numpy(), rec[f"final:{k}"]), k
    assert _digest([v.detach().numpy() for v in p.values()]) == str(rec["final_digest"])


@pytest.mark.parametrize("tag", ["a3k5d35", "a2k8d20"])
def test_fixture_cases_stay_off_the_clip_and_match_the_fp64_restatement(tag):
    actors, obs, action, lpo, adv, index, ent_coef, rec = UA.golden_case(_npz("g_actor_per_agent"), _npz("g_policy"), tag)
    r = UA.loss_and_grad(actors, obs, action, lpo, adv, index, entropy_coef=ent_coef)
    assert U.assert_off_the_clip(r) > 0.03
    scale = max(1.0, np.abs(r["adv"]).max())
    assert abs(r["policy_loss"] - float(rec["u1:policy_loss"])) <= 1e-5 * scale
    assert abs(r["entropy"] - float(rec["u1:entropy"])) <= 1e-5 and abs(r["ess"] - float(rec["u1:ESS"])) <= 1e-5
    assert abs(r["grad_norm"] - float(rec["u1:grad_norm"])) <= 1e-4 * r["grad_norm"]
    # the entropy share: each agent's d log_std carries -entropy_coef / A beside its rows' part
    r0 = UA.loss_and_grad(actors, obs, action, lpo, adv, index, entropy_coef=0.0)
    A = obs["state_self"].shape[1]
    assert np.abs((r["grads"]["act_dist.log_std"] - r0["grads"]["act_dist.log_std"]) + ent_coef / A).max() <= 1e-12


def _nets(A, D=20, seed=0):
    actors, critic = P.random_parameters_per_agent(D, A, seed)
    g = torch.Generator().manual_seed(seed + 1)
    return {k: v + torch.randn(v.shape, generator=g) * 0.05 for k, v in actors.items()}, critic


def _obs(E, A, K, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(E, A, D, generator=g), torch.randn(E, A, A - 1, 3, generator=g) if A > 1 else None, torch.randn(E, A, K, 5, generator=g))


@pytest.mark.parametrize("A", [3, 1])
def test_cpu_forward_of_agent_a_is_torch_forward_with_slice_a_exactly(A):
    actors, critic = _nets(A)
    xs, xo, xc = _obs(9, A, 4, 20, 2)
    pol = P.PerAgentDevicePolicy(actors, critic, cfg={"share_actor": False})
    assert pol.per_agent and pol.num_agents == A and tuple(pol.scale.shape) == (A, 4) and pol.has_others == (A > 1)
    eps = torch.randn(9, A, 4, generator=torch.Generator().manual_seed(3))
    outs = {"eps": pol.forward(xs, xo, xc, eps=eps), "mode": pol.forward(xs, xo, xc, deterministic=True)}
    assert torch.equal(pol.act(xs, xo, xc), outs["mode"].action)
    val = pol.forward(xs, xo, xc, value_only=True)
    assert val.action is None and torch.equal(val.value, outs["eps"].value)
    crit = P.parse_parameters(critic, P.CRITIC_NAMES, "critic")
    for a in range(A):
        sl = P.agent_slice(pol.actor_p, a)
        want = {"eps": P.torch_forward(sl, crit, xs.unsqueeze(2), xo, xc, eps), "mode": P.torch_forward(sl, crit, xs.unsqueeze(2), xo, xc, deterministic=True)}
        for k in outs:
            for f in ("action", "log_prob", "value", "loc"):
                assert torch.equal(getattr(outs[k], f)[:, a], getattr(want[k], f)[:, a]), (k, f, a)
    if A > 1:
        assert not torch.equal(outs["mode"].action[:, 0], P.torch_forward(P.agent_slice(pol.actor_p, 1), crit, xs.unsqueeze(2), xo, xc,
                                                                          deterministic=True).action[:, 0])


def test_parsing_stacked_mapping_module_prefix_checkpoint_and_one_agent(tmp_path):
    actors, critic = _nets(3)
    xs, xo, xc = _obs(4, 3, 4, 20, 5)
    want = P.PerAgentDevicePolicy(actors, critic).forward(xs, xo, xc, deterministic=True)
    prefixed = P.PerAgentDevicePolicy({"module." + k: v for k, v in actors.items()}, {"module." + k: v for k, v in critic.items()})
    ckpt = {"actor_params": actors, "critic": critic, "value_normalizer": {}}
    path = tmp_path / "checkpoint.pt"
    torch.save(ckpt, path)
    for pol in (prefixed, P.PerAgentDevicePolicy.from_checkpoint(ckpt), P.PerAgentDevicePolicy.from_checkpoint(str(path), cfg={"share_actor": False})):
        assert isinstance(pol, P.PerAgentDevicePolicy) and torch.equal(pol.forward(xs, xo, xc, deterministic=True).action, want.action)
    one, crit1 = _nets(1)
    assert not any("state_others" in k for k in one)             # absent at A = 1
    pol1 = P.PerAgentDevicePolicy(one, crit1)
    xs1, _, xc1 = _obs(4, 1, 4, 20, 6)
    assert pol1.forward(xs1, None, xc1).action.shape == (4, 1, 4)
    td = {("agents", "observation"): {"state_self": xs, "state_others": xo, "cylinders": xc}}
    assert torch.equal(P.PerAgentDevicePolicy(actors, critic).value(td), want.value)      # the inherited value_op


def test_every_refusal_comes_before_anything_is_built(monkeypatch):
    actors, critic = _nets(3)
    shared, _ = P.random_parameters(20, 3, 0)
    monkeypatch.setattr(abi, "load_library", lambda: pytest.fail("a refused configuration must not load the library"))
    bad_cfgs = [({"share_actor": True}, P.PolicyConfigError), ({"share_actor": False, "critic_input": "state"}, P.PolicyConfigError),
                ({"share_actor": False, "actor": {"rnn": {"cls": "gru"}}}, P.PolicyConfigError), ({"share_actor": False, "critic": {"rnn": {"cls": "gru"}}}, P.PolicyConfigError),
                ({"share_actor": False, "actor": {"tanh": True}}, P.PolicyConfigError)]
    for cfg, exc in bad_cfgs:
        with pytest.raises(exc):
            P.PerAgentDevicePolicy(actors, critic, cfg=cfg)
        with pytest.raises(exc):
            learner.PerAgentDeviceLearner(actors, critic, cfg)
        with pytest.raises(exc):
            AT.make_optimizer_per_agent(actors, cfg)
    for cfg, exc in (({"share_actor": False, "actor": {"weight_decay": 0.01}}, NotImplementedError),
                     ({"share_actor": False, "actor": {"lr_scheduler": "x"}}, P.PolicyConfigError)):
        with pytest.raises(exc):
            learner.PerAgentDeviceLearner(actors, critic, cfg)
        with pytest.raises(exc):
            AT.make_optimizer_per_agent(actors, cfg)
    with pytest.raises(P.PolicyConfigError, match="no leading agent dimension"):
        P.PerAgentDevicePolicy(shared, critic)
    ragged = dict(actors)
    ragged["act_dist.log_std"] = actors["act_dist.log_std"][:2]
    with pytest.raises(P.PolicyConfigError, match="leading agent dimension"):
        P.PerAgentDevicePolicy(ragged, critic)
    with pytest.raises(P.PolicyConfigError):                     # a recurrent actor's tensors
        P.PerAgentDevicePolicy({**actors, "rnn.cell.weight_ih": torch.zeros(3, 384, 128)}, critic)
    pol = P.PerAgentDevicePolicy(actors, critic)
    xs, xo, xc = _obs(4, 2, 4, 20, 7)
    with pytest.raises(ValueError):                              # the observation's A disagrees with the stacked tensors'
        pol.forward(xs, torch.zeros(4, 2, 2, 3), xc)
    with pytest.raises(NotImplementedError):
        learner.PerAgentDeviceLearner(actors, critic, {"share_actor": False}, group="world")
    rec = type("R", (), {"recurrent": True})()
    with pytest.raises(P.PolicyConfigError):
        learner.PerAgentDeviceLearner(actors, critic, {"share_actor": False}, device_policy=rec)
    with pytest.raises(P.PolicyConfigError):
        learner.PerAgentDeviceLearner(actors, critic, {"share_actor": False}, device_policy=P.DevicePolicy(shared, critic))
    # the update's refusals leave no .grad behind
    p = {k: torch.nn.Parameter(v.clone()) for k, v in actors.items()}
    xs, xo, xc = _obs(6, 3, 4, 20, 8)
    act, lp = torch.zeros(6, 3, 4), torch.zeros(6, 3, 1)
    calls = [lambda: AT.update_actor_per_agent(p, xs, xo, xc, act, lp, lp, AT.make_optimizer_per_agent(p), cfg={"share_actor": True}),
             lambda: AT.update_actor_per_agent(p, xs, xo, xc, act, lp, lp, torch.optim.Adam(p.values())),
             lambda: AT.policy_loss_and_grad_per_agent(p, xs, xo, xc, act, lp, lp, clip_param=-1.0),
             lambda: AT.policy_loss_and_grad_per_agent(p, xs[:, :2], xo[:, :2, :1], xc[:, :2], act[:, :2], lp[:, :2], lp[:, :2]),
             lambda: AT.policy_loss_and_grad_per_agent(p, xs, xo, xc, act, lp, lp, index=torch.tensor([7]), check_index=True),
             lambda: AT.policy_loss_and_grad_per_agent({k: v for k, v in shared.items()}, xs, xo, xc, act, lp, lp)]
    for call in calls:
        with pytest.raises((ValueError, TypeError, IndexError, P.PolicyConfigError)):
            call()
    assert all(v.grad is None for v in p.values())


def test_the_existing_classes_still_refuse_stacked_parameters():
    actors, critic = _nets(3)
    xs, xo, xc = _obs(6, 3, 4, 20, 9)
    with pytest.raises(P.PolicyConfigError):
        P.DevicePolicy(actors, critic)
    with pytest.raises(P.PolicyConfigError):
        P.DevicePolicy(P.random_parameters(20, 3, 0)[0], critic, cfg={"share_actor": False})
    with pytest.raises(P.PolicyConfigError):
        P.RecurrentDevicePolicy({**actors, **{k: v.unsqueeze(0).repeat(3, *[1] * v.dim()) for k, v in P.random_rnn_parameters().items()}},
                                {**critic, **P.random_rnn_parameters(1)})
    with pytest.raises(P.PolicyConfigError):
        AT.policy_loss_and_grad(actors, xs, xo, xc, torch.zeros(6, 3, 4), torch.zeros(6, 3, 1), torch.zeros(6, 3, 1))
    with pytest.raises(P.PolicyConfigError):
        AT.make_optimizer(actors)
    with pytest.raises(P.PolicyConfigError):
        learner.DeviceLearner(actors, critic, {"share_actor": False})
    with pytest.raises(P.PolicyConfigError):
        learner.DeviceLearner(actors, critic, None)
    with pytest.raises(ValueError):                              # (the op's own refusal of a shape it does not take)
        ENC.encode({P._ENCODER[k[len("encoder."):]]: v for k, v in actors.items() if k.startswith("encoder.")}, xs, xo, xc)


@pytest.mark.parametrize("use_tp", [True, False])
def test_learner_on_cpu_tensors_is_the_hand_driven_sequence_bit_for_bit(use_tp):
    """A two-minibatch train_rollout (2 epochs) against the same sequence driven by hand through the public calls; state_dict round-trips."""
    N, T, A = 8, 8, 3
    start = PC.make_state(A, 41)
    ro = PC.make_rollout(start, N, T, A, 42)
    kw = {k: v for k, v in ro.items() if k != "tp"} | ({"tp": ro["tp"]} if use_tp else {})
    hand_state = PC.clone_state(start)
    opts = PC.hand_optimisers(hand_state)
    hand = PC.hand_train_op(hand_state, opts, ro, torch.Generator().manual_seed(5), use_tp=use_tp)
    state = PC.clone_state(start)
    L = PC.make_learner(state, seed=5, use_tp=use_tp)
    assert isinstance(L.policy, P.PerAgentDevicePolicy)
    info = L.train_rollout(**kw)
    if not use_tp:
        opts["tp"] = None
    LC.assert_same_state(LC.state_tensors(state, LC.learner_opts(L)), LC.state_tensors(hand_state, opts), "train_rollout against the hand sequence")
    PC.check_info(info, hand, use_tp)
    assert set(info) == {f"drone/{k}" for k in learner.INFO_KEYS if use_tp or k != "TP_loss"}
    # state_dict: the reference's entries with the STACKED actor_params, and back into a fresh learner bit for bit
    sd = copy.deepcopy(L.state_dict())
    assert all(v.shape[0] == A for v in sd["actor_params"].values())
    fresh = PC.clone_state(PC.make_state(A, 99))
    L2 = PC.make_learner(fresh, seed=5, use_tp=use_tp)
    L2.load_state_dict(sd)
    held = lambda st, Lr: {k: v for k, v in LC.state_tensors(st, LC.learner_opts(Lr)).items() if use_tp or not k.startswith("tp.")}   # noqa: E731
    LC.assert_same_state(held(fresh, L2), held(state, L), "state_dict round trip")
    pol = P.PerAgentDevicePolicy.from_checkpoint(sd)             # the checkpoint dict is the policy's source too
    assert all(torch.equal(pol.actor_p[P.ACTOR_NAMES[k]], v) for k, v in sd["actor_params"].items())


def test_c_entries_refuse_bad_arguments_without_a_device():
    import __graft_entry__ as g
    lib = C.CDLL(g.build())
    lib.hns_policy_packed_agents_bytes.restype = C.c_size_t
    lib.hns_policy_packed_agents_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.hns_policy_packed_bytes.restype = C.c_size_t
    one = lib.hns_policy_packed_bytes(C.c_int32(35)) // 2
    assert [lib.hns_policy_packed_agents_bytes(35, a) for a in (1, 3, 7)] == [2 * one, 4 * one, 8 * one]
    assert [lib.hns_policy_packed_agents_bytes(d, a) for d, a in ((0, 3), (97, 3), (35, 0), (35, 8))] == [0, 0, 0, 0]
    lib.hns_actor_train_agents_workspace_bytes.restype = C.c_size_t
    lib.hns_actor_train_agents_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.hns_actor_train_workspace_bytes.restype = C.c_size_t
    lib.hns_actor_train_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    assert lib.hns_actor_train_agents_workspace_bytes(24576, 35, 3, 5) > 0
    assert [lib.hns_actor_train_agents_workspace_bytes(r, d, a, k) for r, d, a, k in ((0, 35, 3, 5), (10, 35, 3, 5), (9, 97, 3, 5), (9, 35, 8, 5), (9, 35, 3, 17))] == [0] * 5
    # an agent's tiles are padded to whole row ranges: at most one range's tiles per agent beyond the shared layout, never less than it
    shared, agents = lib.hns_actor_train_workspace_bytes(786432, 35, 3, 5), lib.hns_actor_train_agents_workspace_bytes(786432, 35, 3, 5)
    assert shared <= agents <= 1.01 * shared
    lib.hns_last_error.restype = C.c_char_p
    net, io = abi.HnsPolicyNet(), abi.HnsPolicyIo()
    assert lib.hns_policy_pack_agents(C.byref(net), C.byref(net), 35, 9, None, None) == abi.HNS_ERR_INVALID_ARG and b"num_agents" in lib.hns_last_error()
    assert lib.hns_policy_pack_agents(C.byref(net), C.byref(net), 35, 3, None, None) == abi.HNS_ERR_INVALID_ARG and b"packed image" in lib.hns_last_error()
    lib.hns_policy_forward_agents.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p]
    assert lib.hns_policy_forward_agents(None, 35, 8, 3, 5, C.byref(io), 0, 0, None, None) == abi.HNS_ERR_INVALID_ARG
    assert b"hns_policy_forward_agents" in lib.hns_last_error()
    lib.hns_policy_act_agents.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    assert lib.hns_policy_act_agents(None, 35, 8, 3, 5, C.byref(io), None) == abi.HNS_ERR_INVALID_ARG and b"hns_policy_act_agents" in lib.hns_last_error()
    b = abi.HnsActorBatch()
    lib.hns_actor_train_grad_agents.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p] + [C.c_void_p] * 6 + \
        [C.c_size_t, C.c_void_p]
    assert lib.hns_actor_train_grad_agents(C.byref(net), C.byref(b), 35, 3, 5, 0.1, 0.001, C.byref(net), None, None, None, None, None, None, 0, None) == \
        abi.HNS_ERR_INVALID_ARG and b"null pointer" in lib.hns_last_error()
