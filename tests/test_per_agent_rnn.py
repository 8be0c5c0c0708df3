"""Recurrent per-agent actors (share_actor: False with actor.rnn / critic.rnn), CPU part: the CPU path of
hns_amd.policy.PerAgentRecurrentDevicePolicy against the reference's own stacked recurrent actor (tests/golden/g_policy_rnn_per_agent.npz), its
restatement property (row (e, a) is `torch_forward_rnn` with slice a, bit for bit), its parsing and refusals, the learners' refusals, the
checkpoint round trip, the collector on test_collector.py's stub env, and the C entries' refusals (they come before any launch, so they run
without a device)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import per_agent_rnn_cases as PR
import policy_rnn_reference as RR
from hns_amd import abi, collector, learner
from hns_amd import policy as P
from hns_amd.tensordict_shim import _ShimTensorDict as TD
from test_collector import StubEnv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RNN_CFG = {"share_actor": False, "critic_input": "obs", "actor": {"rnn": {"cls": "gru"}}, "critic": {"rnn": {"cls": "gru"}}}


@pytest.fixture(scope="module")
def goldens():
    return tuple(np.load(os.path.join(GOLDEN, n)) for n in ("g_policy.npz", "g_gru.npz", "g_policy_rnn_per_agent.npz"))


def _t(d):
    return {k: torch.as_tensor(np.asarray(v)) for k, v in d.items()}


def _obs(o):
    return torch.as_tensor(o["state_self"]), torch.as_tensor(o["state_others"]) if "state_others" in o else None, torch.as_tensor(o["cylinders"])


def _nets(A, D=20, seed=0):
    actors, critic = PR.random_net(D, A, seed)
    return _t(actors), _t(critic)


def _rand_obs(E, A, K, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(E, A, D, generator=g), torch.randn(E, A, A - 1, 3, generator=g) if A > 1 else None, torch.randn(E, A, K, 5, generator=g))


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", PR.CASES)
def test_the_cpu_path_reproduces_the_references_stacked_recurrent_actor(goldens, tag):
    """Chained through the CPU path's own states, at the tolerance test_policy_rnn.py applies to g_policy_rnn.npz.  The file's generator
    asserted that another agent's slice moves loc by at least 100 times that."""
    gp, gg, z = goldens
    actors, critic, case = PR.golden_case(z, gp, gg, tag)
    pol = P.PerAgentRecurrentDevicePolicy(_t(actors), _t(critic), cfg=RNN_CFG)
    assert pol.recurrent is True and pol.per_agent is True
    E, A, K, D, T = (int(v) for v in case["shape"])
    assert (E, A, K, D, T) == ((11, 3, 5, 35, 5) if tag == "a3k5d35" else (4, 2, 8, 20, 3)) and pol.num_agents == A
    assert case["is_init"][0].any() and not case["is_init"][0].all() and case["is_init"][3 if T == 5 else 0].any()
    ha, hc = torch.as_tensor(case["h0:actor"]), torch.as_tensor(case["h0:critic"])
    for t in range(T):
        out = pol.forward(*_obs(RR.step_obs(case, t)), actor_state=ha, critic_state=hc, is_init=torch.as_tensor(case["is_init"][t]),
                          eps=torch.as_tensor(case["eps"][t]))
        for name in ("loc", "action", "log_prob", "value", "actor_state", "critic_state"):
            err = float((getattr(out, name) - torch.as_tensor(case[name][t])).abs().max())
            assert err <= PR.GOLDEN_TOL, (tag, t, name, err)
        ha, hc = out.actor_state, out.critic_state
    # the test-side fp64 restatement per slice (the GPU gate's yardstick) agrees with the reference too
    ref = PR.slice_forward(actors, critic, RR.step_obs(case, 0), case["h0:actor"], case["h0:critic"], case["is_init"][0], case["eps"][0],
                           torch.float64)
    for name in PR.OUTPUTS:
        assert float(np.abs(ref[name] - case[name][0]).max()) <= PR.GOLDEN_TOL, name


@pytest.mark.parametrize("A", [3, 1])
def test_cpu_row_of_agent_a_is_torch_forward_rnn_with_slice_a_exactly(A):
    E, K, D = 9, 4, 20
    actors, critic = _nets(A, D, 3)
    xs, xo, xc = _rand_obs(E, A, K, D, 2)
    pol = P.PerAgentRecurrentDevicePolicy(actors, critic, cfg=RNN_CFG)
    assert pol.num_agents == A and tuple(pol.scale.shape) == (A, 4) and pol.has_others == (A > 1)
    assert pol.actor_rnn["weight_ih"].shape == (A, 384, 128) and pol.critic_rnn["weight_ih"].shape == (384, 128)
    assert pol.actor_rnn["weight_ih"].data_ptr() == actors["rnn.cell.weight_ih"].data_ptr()          # read in place
    g = torch.Generator().manual_seed(3)
    eps, ha, hc = torch.randn(E, A, 4, generator=g), 0.5 * torch.randn(E, A, 128, generator=g), 0.5 * torch.randn(E, A, 128, generator=g)
    flags = torch.as_tensor(PR.random_flags(E, 4))
    kw = dict(actor_state=ha, critic_state=hc, is_init=flags)
    outs = {"eps": pol.forward(xs, xo, xc, eps=eps, **kw), "mode": pol.forward(xs, xo, xc, deterministic=True, **kw)}
    action, state = pol.act_step(xs, xo, xc, state=ha, is_init=flags)
    assert torch.equal(action, outs["mode"].action) and torch.equal(state, outs["mode"].actor_state)
    val = pol.forward(xs, xo, xc, critic_state=hc, is_init=flags, value_only=True)
    assert val.action is None and val.actor_state is None and torch.equal(val.value, outs["eps"].value)
    assert torch.equal(val.critic_state, outs["eps"].critic_state)
    for a in range(A):
        sl = P.RecurrentDevicePolicy({k: v[a] for k, v in actors.items()}, critic)
        want = {"eps": sl.forward(xs, xo, xc, eps=eps, **kw), "mode": sl.forward(xs, xo, xc, deterministic=True, **kw)}
        for k in outs:
            for f in P.RecurrentPolicyOutput._fields:
                assert torch.equal(getattr(outs[k], f)[:, a], getattr(want[k], f)[:, a]), (k, f, a)
        wa, ws = sl.act_step(xs, xo, xc, state=ha, is_init=flags)
        assert torch.equal(action[:, a], wa[:, a]) and torch.equal(state[:, a], ws[:, a])
    if A > 1:                                                    # the slices are not interchangeable
        other = P.RecurrentDevicePolicy({k: v[1] for k, v in actors.items()}, critic).forward(xs, xo, xc, deterministic=True, **kw)
        assert not torch.equal(outs["mode"].action[:, 0], other.action[:, 0]) and not torch.equal(outs["mode"].actor_state[:, 0], other.actor_state[:, 0])
    # in place, and the states None: zeros
    ia, ic = ha.clone(), hc.clone()
    got = pol.forward(xs, xo, xc, actor_state=ia, critic_state=ic, is_init=flags, eps=eps, out_states=(ia, ic))
    assert got.actor_state is ia and torch.equal(ia, outs["eps"].actor_state) and torch.equal(ic, outs["eps"].critic_state)
    z = torch.zeros(E, A, 128)
    assert torch.equal(pol.forward(xs, xo, xc, deterministic=True).loc, pol.forward(xs, xo, xc, actor_state=z, critic_state=z, deterministic=True).loc)


def test_parsing_module_prefix_checkpoint_round_trip_and_the_references_keys(tmp_path):
    A = 3
    actors, critic = _nets(A, 20, 5)
    xs, xo, xc = _rand_obs(4, A, 4, 20, 5)
    want = P.PerAgentRecurrentDevicePolicy(actors, critic).forward(xs, xo, xc, deterministic=True)
    prefixed = P.PerAgentRecurrentDevicePolicy({"module." + k: v for k, v in actors.items()}, {"module." + k: v for k, v in critic.items()})
    ckpt = {"actor_params": actors, "critic": critic, "value_normalizer": {}}
    path = tmp_path / "checkpoint.pt"
    torch.save(ckpt, path)
    for pol in (prefixed, P.PerAgentRecurrentDevicePolicy.from_checkpoint(ckpt),
                P.PerAgentRecurrentDevicePolicy.from_checkpoint(str(path), cfg=RNN_CFG)):
        assert isinstance(pol, P.PerAgentRecurrentDevicePolicy)
        got = pol.forward(xs, xo, xc, deterministic=True)
        assert all(torch.equal(getattr(got, f), getattr(want, f)) for f in got._fields)
    with pytest.raises(KeyError):
        P.PerAgentRecurrentDevicePolicy.from_checkpoint({"actor_params": actors})
    # __call__ and value: the reference's keys
    pol = P.PerAgentRecurrentDevicePolicy(actors, critic)
    ha, hc = 0.5 * torch.randn(4, A, 128), 0.5 * torch.randn(4, A, 128)
    td = {("agents", "observation"): {"state_self": xs, "state_others": xo, "cylinders": xc}, "drone.actor_rnn_state": ha,
          "drone.critic_rnn_state": hc, "is_init": torch.tensor([[True], [False], [False], [True]])}
    value = pol.value(td)
    full = pol.forward(xs, xo, xc, actor_state=ha, critic_state=hc, is_init=td["is_init"], deterministic=True)
    pol(td, deterministic=True)
    assert torch.equal(td[("agents", "action")], full.loc) and torch.equal(td["drone.actor_rnn_state"], full.actor_state)
    assert torch.equal(td["state_value"], full.value) and torch.equal(value, full.value) and torch.equal(td["drone.critic_rnn_state"], full.critic_state)
    assert td["drone.action_logp"].shape == (4, A, 1)
    # random_rnn_parameters_per_agent: stacked, the reference's names, no two agents alike
    r = P.random_rnn_parameters_per_agent(A, 7)
    assert set(r) == {"rnn." + n for n in RR.GRU_NAMES} and r["rnn.cell.weight_hh"].shape == (A, 384, 128)
    assert not torch.equal(r["rnn.cell.weight_hh"][0], r["rnn.cell.weight_hh"][1])
    shared_a, shared_c = P.random_parameters_per_agent(20, A, 1)
    P.PerAgentRecurrentDevicePolicy({**shared_a, **r}, {**shared_c, **P.random_rnn_parameters(2)})


def test_every_refusal_comes_before_anything_is_built(monkeypatch):
    A = 3
    actors, critic = _nets(A, 20, 6)
    monkeypatch.setattr(abi, "load_library", lambda: pytest.fail("a refused configuration must not load the library"))
    plain_a = {k: v for k, v in actors.items() if not k.startswith("rnn.")}
    plain_c = {k: v for k, v in critic.items() if not k.startswith("rnn.")}
    for cfg in ({**RNN_CFG, "share_actor": True}, {**RNN_CFG, "critic_input": "state"}, {**RNN_CFG, "actor": {"rnn": {"cls": "gru"}, "tanh": True}}):
        with pytest.raises(P.PolicyConfigError):
            P.PerAgentRecurrentDevicePolicy(actors, critic, cfg=cfg)
    with pytest.raises(P.PolicyConfigError, match="share_actor"):
        P.PerAgentRecurrentDevicePolicy(actors, critic, cfg={"share_actor": True})
    shared = {k: v[0] for k, v in actors.items()}
    with pytest.raises(P.PolicyConfigError, match="no leading agent dimension"):                 # nothing stacked
        P.PerAgentRecurrentDevicePolicy(shared, critic)
    with pytest.raises(P.PolicyConfigError, match="no leading agent dimension"):                 # the actor stacked, its GRU not
        P.PerAgentRecurrentDevicePolicy({**actors, **{k: v[0] for k, v in actors.items() if k.startswith("rnn.")}}, critic)
    with pytest.raises(P.PolicyConfigError, match="no leading agent dimension"):                 # the GRU stacked, the actor not
        P.PerAgentRecurrentDevicePolicy({**shared, **{k: v for k, v in actors.items() if k.startswith("rnn.")}}, critic)
    ragged = dict(actors)
    ragged["rnn.layer_norm.bias"] = actors["rnn.layer_norm.bias"][:2]
    with pytest.raises(P.PolicyConfigError, match="leading agent dimension"):
        P.PerAgentRecurrentDevicePolicy(ragged, critic)
    ragged = dict(actors)
    ragged["act_dist.log_std"] = actors["act_dist.log_std"][:2]
    with pytest.raises(P.PolicyConfigError, match="leading agent dimension"):
        P.PerAgentRecurrentDevicePolicy(ragged, critic)
    two = {k: (v[:2] if k.startswith("rnn.") else v) for k, v in actors.items()}                 # three actors with two GRUs
    with pytest.raises(P.PolicyConfigError):
        P.PerAgentRecurrentDevicePolicy(two, critic)
    wide = dict(actors)
    wide["rnn.cell.weight_hh"] = torch.zeros(A, 3 * 64, 64)
    with pytest.raises(P.PolicyConfigError, match="GRUCell"):
        P.PerAgentRecurrentDevicePolicy(wide, critic)
    with pytest.raises(P.PolicyConfigError, match="no GRU"):                                     # an rnn on only one of the two networks
        P.PerAgentRecurrentDevicePolicy(actors, plain_c)
    with pytest.raises(P.PolicyConfigError, match="no GRU"):
        P.PerAgentRecurrentDevicePolicy(plain_a, critic)
    with pytest.raises(P.PolicyConfigError, match="critic"):                                     # a critic with stacked tensors
        P.PerAgentRecurrentDevicePolicy(actors, {k: v.unsqueeze(0).repeat(A, *[1] * v.dim()) for k, v in critic.items()})
    extra = dict(actors)
    extra["rnn.cell.weight_hr"] = torch.zeros(A, 4)
    with pytest.raises(P.PolicyConfigError, match="weight_hr"):
        P.PerAgentRecurrentDevicePolicy(extra, critic)
    with pytest.raises(TypeError):
        P.PerAgentRecurrentDevicePolicy({k: v.double() for k, v in actors.items()}, critic)
    pol = P.PerAgentRecurrentDevicePolicy(actors, critic)
    xs, xo, xc = _rand_obs(4, 2, 4, 20, 7)
    with pytest.raises(ValueError, match="agents"):              # the observation's A disagrees with the stacked tensors'
        pol.forward(xs, xo, xc)
    with pytest.raises(ValueError, match="agents"):
        pol.act_step(xs, xo, xc)
    xs, xo, xc = _rand_obs(4, A, 4, 20, 7)
    with pytest.raises(ValueError):
        pol.forward(xs, xo, xc, actor_state=torch.zeros(4, A, 64))
    with pytest.raises(ValueError):
        pol.forward(xs, xo, xc, is_init=torch.zeros(5, dtype=torch.bool))
    with pytest.raises(P.PolicyConfigError, match="deterministic"):
        pol.act(xs, xo, xc)


def test_no_learner_trains_it_and_the_existing_classes_refuse_what_they_refused():
    A = 3
    actors, critic = _nets(A, 20, 8)
    pol = P.PerAgentRecurrentDevicePolicy(actors, critic)
    shared_rnn = {k: v[0] for k, v in actors.items()}
    plain_a = {k: v for k, v in actors.items() if not k.startswith("rnn.")}
    plain_c = {k: v for k, v in critic.items() if not k.startswith("rnn.")}
    cfg = {"actor": {"rnn": {"cls": "gru"}}, "critic": {"rnn": {"cls": "gru"}}}
    # the two recurrent learners: a per_agent policy, or stacked actor tensors, name the open item
    for make in (lambda **kw: learner.RecurrentDeviceLearner(kw.pop("actor", shared_rnn), critic, cfg, **kw),
                 lambda **kw: learner.DataParallelRecurrentLearner(kw.pop("actor", shared_rnn), critic, cfg, group="world", **kw)):
        with pytest.raises(P.PolicyConfigError, match="open item"):
            make(device_policy=pol)
        with pytest.raises(P.PolicyConfigError, match="open item"):
            make(actor=actors)
        with pytest.raises(P.PolicyConfigError, match="open item"):
            make(device_policy=type("R", (), {"recurrent": True, "per_agent": True})())
        with pytest.raises(P.PolicyConfigError, match="RecurrentDevicePolicy"):      # ... and what they refused before, as before
            make(device_policy=P.DevicePolicy({k: v[0] for k, v in plain_a.items()}, plain_c))
    with pytest.raises(NotImplementedError):
        learner.RecurrentDeviceLearner(shared_rnn, critic, cfg, group="world")
    with pytest.raises(ValueError, match="group"):
        learner.DataParallelRecurrentLearner(shared_rnn, critic, cfg)
    # the other two learners
    with pytest.raises(P.PolicyConfigError, match="recurrent"):
        learner.DeviceLearner(None, None, {}, device_policy=pol)
    with pytest.raises(P.PolicyConfigError, match="recurrent"):
        learner.PerAgentDeviceLearner(plain_a, plain_c, {"share_actor": False}, device_policy=pol)
    with pytest.raises(P.PolicyConfigError):
        learner.PerAgentDeviceLearner(actors, critic, {"share_actor": False})
    with pytest.raises(P.PolicyConfigError):
        learner.DeviceLearner(actors, critic, {"share_actor": False})
    # the three existing policies
    with pytest.raises(P.PolicyConfigError):
        P.RecurrentDevicePolicy(actors, critic)
    with pytest.raises(P.PolicyConfigError):
        P.RecurrentDevicePolicy(shared_rnn, critic, cfg={"share_actor": False})
    with pytest.raises(P.PolicyConfigError):
        P.PerAgentDevicePolicy(actors, critic)
    with pytest.raises(P.PolicyConfigError):
        P.PerAgentDevicePolicy(plain_a, plain_c, cfg=RNN_CFG)
    with pytest.raises(P.PolicyConfigError):
        P.DevicePolicy(actors, critic)
    P.RecurrentDevicePolicy(shared_rnn, critic)                  # (the slice is a shared recurrent actor)
    P.PerAgentDevicePolicy(plain_a, plain_c)


def test_the_collector_takes_the_policy_unchanged_on_the_stub_env():
    """DeviceCollector dispatches on policy.recurrent: the rollout it stores equals a hand loop over policy.forward, states and flags included."""
    A, T, L = 3, 8, 4
    lengths = [5, 5, 7]
    actors, critic = _nets(A, 3, 9)
    make = lambda: P.PerAgentRecurrentDevicePolicy(actors, critic, seed=5)          # noqa: E731
    env, pol = StubEnv(lengths, A), make()
    col = collector.DeviceCollector(env, pol, T, rnn_seq_len=L)
    st = col.collect()
    rk = st.recurrent_kwargs()
    N = len(lengths)
    assert rk["actor_rnn_state"].shape == rk["critic_rnn_state"].shape == (N, T // L, A, 128) and rk["rnn_seq_len"] == L
    assert bool(st.data["is_init"][:, 0].all()) and bool(st.data["done"][0, 4]) and not bool(st.data["done"][2, 4])
    # the hand loop: a second env and a second policy of the same seed (the CPU generator draws the same noise)
    env2, pol2 = StubEnv(lengths, A), make()
    cur = env2.reset()
    ha = hc = torch.zeros(N, A, 128)
    flags = torch.ones(N, 1, dtype=torch.bool)
    for t in range(T):
        obs = cur[("agents", "observation")]
        if t % L == 0:
            assert torch.equal(rk["actor_rnn_state"][:, t // L], ha) and torch.equal(rk["critic_rnn_state"][:, t // L], hc), t
        out = pol2.forward(obs["state_self"], obs["state_others"], obs["cylinders"], actor_state=ha, critic_state=hc, is_init=flags)
        for k, v in (("action", out.action), ("log_probs", out.log_prob), ("state_value", out.value), ("is_init", flags)):
            assert torch.equal(st.data[k][:, t], v), (k, t)
        ha, hc = out.actor_state, out.critic_state
        nxt = env2.step(TD({"agents": {"action": out.action}}, env2.batch_size))["next"]
        done = nxt["done"].as_subclass(torch.Tensor).clone()
        flags = done
        cur = env2.reset(TD({"_reset": done}, env2.batch_size)) if bool(done.any()) else nxt
    assert torch.equal(rk["last_critic_rnn_state"], hc) and torch.equal(rk["last_is_init"], flags)
    assert bool(st.data["is_init"][:, 1:].any())                 # an episode boundary inside the rollout


def test_the_abi_declares_the_entries_and_they_refuse_bad_arguments_without_a_device():
    for sym in ("hns_policy_rnn_packed_agents_bytes", "hns_policy_rnn_pack_agents", "hns_policy_forward_rnn_agents", "hns_policy_act_rnn_agents"):
        assert sym in abi.EXPORTED_SYMBOLS
    lib = abi.load_library()
    assert lib.hns_abi_version() == 8
    one = lib.hns_policy_rnn_packed_bytes() // 2
    assert [lib.hns_policy_rnn_packed_agents_bytes(a) for a in (1, 3, 7)] == [2 * one, 4 * one, 8 * one]
    assert [lib.hns_policy_rnn_packed_agents_bytes(a) for a in (0, 8, -1)] == [0, 0, 0]
    err = lambda: lib.hns_last_error().decode()                  # noqa: E731
    bad = abi.HNS_ERR_INVALID_ARG
    n = abi.HnsGruNet()
    img = C.create_string_buffer(64)                             # an aligned non-NULL address: the refusals below come before it is used
    ptr = (C.addressof(img) + 15) & ~15
    assert lib.hns_policy_rnn_pack_agents(C.byref(n), C.byref(n), 0, ptr, None) == bad and "num_agents" in err()
    assert lib.hns_policy_rnn_pack_agents(C.byref(n), C.byref(n), 8, ptr, None) == bad and "num_agents" in err()
    assert lib.hns_policy_rnn_pack_agents(C.byref(n), C.byref(n), 3, None, None) == bad and "packed image" in err()
    assert lib.hns_policy_rnn_pack_agents(C.byref(n), C.byref(n), 3, ptr + 4, None) == bad and "packed image" in err()
    assert lib.hns_policy_rnn_pack_agents(None, C.byref(n), 3, ptr, None) == bad and "null GRU network" in err()
    assert lib.hns_policy_rnn_pack_agents(C.byref(n), C.byref(n), 3, ptr, None) == bad and "GRU parameter" in err()
    assert err().startswith("hns_policy_rnn_pack_agents: ")
    io, rio = abi.HnsPolicyIo(), abi.HnsPolicyRnnIo()
    fwd = lambda packed, rnn, shape=(35, 8, 3, 5), pio=io, prio=rio, flags=0: lib.hns_policy_forward_rnn_agents(  # noqa: E731
        packed, rnn, *shape, C.byref(pio) if pio is not None else None, C.byref(prio) if prio is not None else None, flags, 0, None, None)
    # hns_policy_forward_rnn's order: the packed image / io / shape, the GRU image / rio, the flags, the observation, ...
    assert fwd(None, None) == bad and "packed image / io" in err() and err().startswith("hns_policy_forward_rnn_agents: ")
    assert fwd(ptr, None, pio=None) == bad and "packed image / io" in err()
    assert fwd(ptr, None, shape=(0, 8, 3, 5)) == bad and "self_dim" in err()
    assert fwd(ptr, None, shape=(35, 8, 8, 5)) == bad and "num_agents" in err()
    assert fwd(ptr, None, shape=(35, 8, 3, 17)) == bad and "num_cylinders" in err()
    assert fwd(ptr, None, shape=(35, 0, 3, 5)) == bad and "num_envs" in err()
    assert fwd(ptr, None, flags=4) == bad and "GRU image" in err()
    assert fwd(ptr, ptr + 4) == bad and "GRU image" in err()
    assert fwd(ptr, ptr, prio=None, flags=4) == bad and "rnn io" in err()
    assert fwd(ptr, ptr, flags=4) == bad and "flag" in err()
    assert fwd(ptr, ptr) == bad and "observation" in err()
    act = lambda packed, rnn, shape=(35, 8, 3, 5), pio=io, prio=rio: lib.hns_policy_act_rnn_agents(  # noqa: E731
        packed, rnn, *shape, C.byref(pio) if pio is not None else None, C.byref(prio) if prio is not None else None, None)
    assert act(None, None) == bad and "packed image / io" in err() and err().startswith("hns_policy_act_rnn_agents: ")
    assert act(ptr, None, shape=(35, 8, 0, 5)) == bad and "num_agents" in err()
    assert act(ptr, None) == bad and "GRU image" in err()
    assert act(ptr, ptr, prio=None) == bad and "rnn io" in err()
    assert act(ptr, ptr) == bad and "observation" in err()
