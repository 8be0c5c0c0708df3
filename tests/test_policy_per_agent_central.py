"""Per-agent actors beside the centralised critic (share_actor: False with critic_input: state) on the CPU: PerAgentCentralCriticDevicePolicy's
CPU-tensor path against the two classes it joins (bit for bit) and against the reference's fixture, the refusal matrix, the checkpoint round
trip, and the C entries' size formula and refusals (before any launch, so without a device).  DESIGN.md §7.21."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import central_reference as CR
import policy_reference as R
from hns_amd import abi
from hns_amd import policy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(33, 3, 5, 35), (1, 3, 3, 20), (64, 2, 1, 20), (40, 7, 16, 96), (32, 1, 5, 20)]
E128 = P.EMBED_DIM


def _t(d):
    return {k: torch.as_tensor(v) for k, v in d.items()}


def _obs(E, A, K, D, seed):
    obs, eps = R.random_obs(E, A, K, D, seed)
    return (torch.as_tensor(obs["state_self"]), torch.as_tensor(obs["state_others"]) if A > 1 else None, torch.as_tensor(obs["cylinders"]),
            torch.as_tensor(eps))


def _cfg(**kw):
    return {"share_actor": False, "critic_input": "state", **kw}


@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_path_is_the_two_classes_it_joins(shape):
    """action, log_prob and loc: PerAgentDevicePolicy's CPU bits for the same stacked actor and eps, and for the same seed; value:
    CentralCriticDevicePolicy's CPU bits for the same critic and state, under the fp64 gate; deterministic = act; value_only sets value alone."""
    E, A, K, D = shape
    stacked, obs_critic = P.random_parameters_per_agent(D, A, 3)
    shared_actor = P.random_parameters(D, A, 4)[0]
    critic = CR.random_critic(D, A, 11 + A)
    sd, cyl = (torch.as_tensor(x) for x in CR.random_state(E, A, K, D, 12))
    xs, xo, xc, eps = _obs(E, A, K, D, 13)
    pol = P.PerAgentCentralCriticDevicePolicy(stacked, _t(critic), cfg=_cfg(), seed=5)
    assert pol.per_agent and pol.central and pol.needs_state and not pol.recurrent and pol.num_agents == A
    assert tuple(pol.scale.shape) == (A, 4)
    agents = P.PerAgentDevicePolicy(stacked, obs_critic, seed=5)
    central = P.CentralCriticDevicePolicy(shared_actor, _t(critic), seed=5)
    out, want_a, want_c = pol.forward(xs, xo, xc, sd, cyl, eps=eps), agents.forward(xs, xo, xc, eps=eps), central.forward(xs, xo, xc, sd, cyl, eps=eps)
    for n in ("action", "log_prob", "loc"):
        assert torch.equal(getattr(out, n), getattr(want_a, n)), n
    assert out.value.shape == (E, A, 1) and torch.equal(out.value, want_c.value)
    r64, r32 = (CR.value_np(critic, sd.numpy(), cyl.numpy(), dt) for dt in (torch.float64, torch.float32))
    assert CR.ratio(out.value.numpy(), r64, r32) <= CR.BAR
    a, b = pol.forward(xs, xo, xc, sd, cyl), agents.forward(xs, xo, xc)           # the same seed: the same draw
    assert all(torch.equal(getattr(a, n), getattr(b, n)) for n in ("action", "log_prob", "loc")) and not torch.equal(a.action, out.action)
    det = pol.forward(xs, xo, xc, sd, cyl, deterministic=True)
    assert torch.equal(det.action, det.loc) and torch.equal(det.action, pol.act(xs, xo, xc)) and torch.equal(det.action, agents.act(xs, xo, xc))
    vo = pol.forward(xs, xo, xc, sd, cyl, value_only=True)
    assert vo.action is None and vo.log_prob is None and vo.loc is None and torch.equal(vo.value, out.value)
    # the env's [E, A, K, 5] tensor: agent 0's rows; None: agent 0's rows of the observation's
    wide = cyl.unsqueeze(1).repeat(1, A, 1, 1).contiguous()
    wide[:, 1:] += 1.0
    assert torch.equal(pol.forward(xs, xo, xc, sd, wide, value_only=True).value, out.value)
    assert torch.equal(pol.forward(xs, xo, wide, sd, value_only=True).value, out.value)


def test_agents_rows_come_from_their_own_slices():
    """With actors that differ per agent, agent a's rows differ from what agent b's slice gives them: the identities above could fail."""
    E, A, K, D = 9, 3, 4, 20
    stacked, _ = P.random_parameters_per_agent(D, A, 3)
    critic = P.random_parameters_central(D, A, 3)[1]
    xs, xo, xc, eps = _obs(E, A, K, D, 13)
    sd = torch.randn(E, A, D, generator=torch.Generator().manual_seed(1))
    out = P.PerAgentCentralCriticDevicePolicy(stacked, critic).forward(xs, xo, xc, sd, eps=eps)
    for b in range(A):
        shared = P.CentralCriticDevicePolicy({k: v[b] for k, v in stacked.items()}, critic).forward(xs, xo, xc, sd, eps=eps)
        for a in range(A):
            assert torch.equal(out.loc[:, a], shared.loc[:, a]) == (a == b), (a, b)
        assert torch.equal(out.value, shared.value)


@pytest.mark.parametrize("tag", ("a3k3d35", "a1k3d20", "a4k5d20"))
def test_value_meets_the_reference_fixture_through_the_new_class(tag):
    gc = np.load(os.path.join(ROOT, "tests", "golden", "g_policy_central.npz"))
    critic, sd, cyl, want = CR.golden_case(gc, tag)
    B, A, K, D = (int(x) for x in gc[f"{tag}:shape"])
    xs, xo, xc, _ = _obs(B, A, K, D, 2)
    pol = P.PerAgentCentralCriticDevicePolicy(P.random_parameters_per_agent(D, A, 1)[0], _t(critic))
    got = pol.forward(xs, xo, xc, torch.as_tensor(sd), torch.as_tensor(cyl), value_only=True).value
    np.testing.assert_allclose(got.numpy(), want, atol=1e-5, rtol=1e-5, err_msg=tag)


def test_refusal_matrix():
    """Each raises before anything is built, with the existing exception types; the three existing classes keep their refusals."""
    D, A = 20, 3
    stacked, obs_critic = P.random_parameters_per_agent(D, A, 1)
    actor, critic = P.random_parameters_central(D, A, 1)
    E = P.PolicyConfigError
    new = P.PerAgentCentralCriticDevicePolicy
    ok = new(stacked, critic, cfg=_cfg())
    assert ok.num_agents == A and ok.self_dim == D
    assert new(stacked, critic, cfg={}).num_agents == A and new(stacked, critic, cfg=None).num_agents == A
    for check in (P.check_config_per_agent_central, lambda c: new(stacked, critic, cfg=c)):
        with pytest.raises(E, match="share_actor"):
            check(_cfg(share_actor=True))
        with pytest.raises(E, match="critic_input"):
            check(_cfg(critic_input="obs"))
        with pytest.raises(E, match="rnn"):
            check(_cfg(actor={"rnn": {"cls": "gru"}}))
        with pytest.raises(E, match="rnn"):
            check(_cfg(critic={"rnn": {"cls": "gru"}}))
        with pytest.raises(E, match="tanh"):
            check(_cfg(actor={"tanh": True}))
    with pytest.raises(E, match="no leading agent dimension"):
        new(actor, critic)                                                       # a shared actor
    with pytest.raises(E, match="leading agent dimension"):
        new({**stacked, "act_dist.log_std": stacked["act_dist.log_std"][:2]}, critic)
    with pytest.raises(E, match="state_self|state_others"):
        new(stacked, obs_critic)                                                 # the obs critic's 22 tensors
    with pytest.raises(E, match="state_others"):
        new(stacked, {**critic, "base.split_embed.embed.state_others.weight": torch.zeros(128, 3),
                      "base.split_embed.embed.state_others.bias": torch.zeros(128)})
    with pytest.raises(E, match="rnn"):
        new(stacked, {**critic, **P.random_rnn_parameters(1)})
    with pytest.raises(E, match="rnn"):
        new({**stacked, **P.random_rnn_parameters_per_agent(A, 1)}, critic)
    with pytest.raises(E, match="v_out"):
        new(stacked, P.random_parameters_central(D, 2, 1)[1])                    # two rows beside three actors
    with pytest.raises(E, match="v_out"):
        new(stacked, {**critic, "v_out.weight": torch.zeros(8, 128), "v_out.bias": torch.zeros(8)})
    with pytest.raises(E, match="different widths"):
        new(stacked, P.random_parameters_central(D + 1, A, 1)[1])
    # the three existing classes: unchanged refusals
    with pytest.raises(E, match="leading agent dimension"):
        P.CentralCriticDevicePolicy(stacked, critic)
    with pytest.raises(E, match="share_actor"):
        P.CentralCriticDevicePolicy(actor, critic, cfg=_cfg())
    with pytest.raises(E, match="centralised critic"):
        P.PerAgentDevicePolicy(stacked, obs_critic, cfg=_cfg())
    with pytest.raises(E, match="does not have"):
        P.PerAgentDevicePolicy(stacked, critic)
    with pytest.raises(E):
        P.DevicePolicy(stacked, critic, cfg=_cfg())
    # shapes at the call
    xs, xo, xc, _ = _obs(4, A, 5, D, 2)
    sd = torch.zeros(4, A, D)
    with pytest.raises(ValueError, match="state_drones"):
        ok.forward(xs, xo, xc, sd[:, :2])
    with pytest.raises(ValueError, match="cylinders"):
        ok.forward(xs, xo, xc, sd, torch.zeros(4, 6, 5))
    with pytest.raises(TypeError, match="float32"):
        ok.forward(xs, xo, xc, sd.double())
    with pytest.raises(ValueError, match="agents"):
        new(P.random_parameters_per_agent(D, 2, 1)[0], P.random_parameters_central(D, 2, 1)[1]).forward(xs, xo, xc, sd)


def test_checkpoint_round_trip_and_the_tensordict_calls(tmp_path):
    D, A, E, K = 20, 3, 6, 4
    stacked = P.random_parameters_per_agent(D, A, 4)[0]
    critic = P.random_parameters_central(D, A, 4)[1]
    ck = {"actor_params": {"module." + k: v for k, v in stacked.items()}, "critic": {"module." + k: v for k, v in critic.items()}}
    path = tmp_path / "policy.pt"
    torch.save(ck, path)
    pol = P.PerAgentCentralCriticDevicePolicy.from_checkpoint(str(path), cfg=_cfg())
    for k, f in P.CENTRAL_CRITIC_NAMES.items():
        assert torch.equal(pol.critic_p[f], critic[k]), k
    for k, f in P.ACTOR_NAMES.items():
        assert torch.equal(pol.actor_p[f], stacked[k]) and pol.actor_p[f].shape[0] == A, k
    xs, xo, xc, eps = _obs(E, A, K, D, 6)
    sd = torch.randn(E, A, D, generator=torch.Generator().manual_seed(1))
    a, b = pol.forward(xs, xo, xc, sd, eps=eps), P.PerAgentCentralCriticDevicePolicy(stacked, critic).forward(xs, xo, xc, sd, eps=eps)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for cls in (P.DevicePolicy, P.PerAgentDevicePolicy, P.CentralCriticDevicePolicy):
        with pytest.raises(P.PolicyConfigError):
            cls.from_checkpoint(str(path))
    td = {("agents", "observation"): {"state_self": xs, "state_others": xo, "cylinders": xc}, ("agents", "state"): {"state_drones": sd, "cylinders": xc}}
    want = pol.forward(xs, xo, xc, sd, xc[:, 0].contiguous(), value_only=True).value
    assert torch.equal(pol.value(td), want)
    out = pol(dict(td), deterministic=True)
    assert torch.equal(out["state_value"], want) and out["drone.action_logp"].shape == (E, A, 1)
    assert torch.equal(pol.act(xs, xo, xc), out[("agents", "action")])


def _net(fields, others):
    """An hns_policy_net of never-read, aligned, non-NULL addresses: the refusals below look at the pointers' values alone."""
    n = abi.HnsPolicyNet()
    for f in abi.POLICY_NET_FIELDS:
        if f in fields and (others or "others" not in f):
            setattr(n, f, 0x1000)
    return n


def test_c_entries_size_formula_and_refusals_without_a_device():
    """hns_policy_packed_central_agents_bytes is (A net_floats(D) + central_floats(D)) 4; both new entries refuse, before any launch and in the
    documented order: the two packs' refusals in their order, hns_policy_central_forward's in its order."""
    import __graft_entry__ as g
    lib = C.CDLL(g.build())
    lib.hns_last_error.restype = C.c_char_p
    for name in ("hns_policy_packed_central_agents_bytes", "hns_policy_pack_central_agents", "hns_policy_central_forward_agents"):
        assert name in abi.EXPORTED_SYMBOLS and hasattr(lib, name)
    size = lib.hns_policy_packed_central_agents_bytes
    size.restype, size.argtypes = C.c_size_t, [C.c_int32, C.c_int32]
    net_floats = lambda D: 6 * E128 * E128 + 18 * E128 + 12 + (D + 8) * E128         # noqa: E731  pol_net_floats of csrc/hns_policy.hip
    central_floats = lambda D: 6 * E128 * E128 + 22 * E128 + 8 + (D + 5) * E128      # noqa: E731  pol_central_floats
    for D in (1, 20, 35, 96):
        for A in range(1, 8):
            assert size(D, A) == (A * net_floats(D) + central_floats(D)) * 4, (D, A)
    lib.hns_policy_packed_central_bytes.restype, lib.hns_policy_packed_agents_bytes.restype = C.c_size_t, C.c_size_t
    assert size(35, 1) == lib.hns_policy_packed_central_bytes(C.c_int32(35), C.c_int32(1))
    assert size(35, 3) - size(35, 2) == lib.hns_policy_packed_agents_bytes(C.c_int32(35), C.c_int32(3)) - lib.hns_policy_packed_agents_bytes(C.c_int32(35), C.c_int32(2))
    assert [size(d, a) for d, a in ((0, 3), (97, 3), (35, 0), (35, 8))] == [0, 0, 0, 0]
    bad = abi.HNS_ERR_INVALID_ARG
    err = lambda: lib.hns_last_error().decode()                                     # noqa: E731

    pack = lib.hns_policy_pack_central_agents
    pack.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    actor_fields = set(abi.POLICY_NET_FIELDS)
    critic_fields = actor_fields - {"log_std"}
    actors, critic = _net(actor_fields, True), _net(critic_fields, False)
    img = 0x4000

    def refused(word, a=actors, c=critic, D=35, A=3, packed=img):
        rc = pack(C.byref(a) if a is not None else None, C.byref(c) if c is not None else None, D, A, packed, None)
        assert rc == bad and err().startswith("hns_policy_pack_central_agents: ") and word in err(), (word, rc, err())

    refused("self_dim", D=97, A=9, packed=None)                  # the order: self_dim, num_agents, the image, the actors, the critic
    refused("num_agents", A=9, packed=None)
    refused("packed image", packed=None, a=None)
    refused("packed image", packed=img + 4, a=None)
    refused("null network", a=None, c=None)
    no_others = _net(actor_fields, False)
    refused("state_others embedding missing", a=no_others, c=None)
    refused("log_std", a=_net(critic_fields, True), c=None)
    odd = _net(actor_fields, True)
    odd.ln_w = 0x1002
    refused("non-NULL fp32 array", a=odd, c=None)
    refused("null network", c=None)
    refused("non-NULL fp32 array", c=_net(critic_fields - {"head_b"}, False))
    refused("no state_others embedding", c=_net(critic_fields, True))
    pack(C.byref(no_others), C.byref(_net(critic_fields, True)), 35, 1, img, None)  # one agent: the actor needs no state_others, the critic still must not have one
    assert "no state_others embedding" in err()

    fwd = lib.hns_policy_central_forward_agents
    fwd.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p]

    def io_(**over):
        io = abi.HnsPolicyIo()
        io.obs_self = io.obs_others = io.obs_cylinders = io.action = io.loc = io.log_prob = io.value = 0x1000
        for k, v in over.items():
            if k.endswith("stride"):
                getattr(io, k)[:] = v
            else:
                setattr(io, k, v)
        return io

    def st_(**over):
        st = abi.HnsPolicyState()
        st.state_drones = st.cylinders = 0x1000
        for k, v in over.items():
            if k.endswith("stride"):
                getattr(st, k)[:] = v
            else:
                setattr(st, k, v)
        return st

    def fwd_refused(word, io=None, st=None, packed=img, shape=(35, 8, 3, 5), flags=0, counter=0x2000, no_io=False, no_st=False):
        io, st = io if io is not None else io_(), st if st is not None else st_()
        D, E, A, K = shape
        rc = fwd(packed, D, E, A, K, None if no_io else C.byref(io), None if no_st else C.byref(st), flags, 0, counter, None)
        assert rc == bad and err().startswith("hns_policy_central_forward_agents: ") and word in err(), (word, rc, err())

    fwd_refused("packed image / io", packed=None, shape=(97, 8, 3, 5), flags=4)
    fwd_refused("packed image / io", packed=img + 8, flags=4)
    fwd_refused("packed image / io", no_io=True, flags=4)
    fwd_refused("self_dim", shape=(97, 8, 9, 5), flags=4)
    fwd_refused("num_agents", shape=(35, 8, 8, 17), flags=4)
    fwd_refused("num_cylinders", shape=(35, 0, 3, 17), flags=4)
    fwd_refused("num_envs", shape=(35, 0, 3, 5), flags=4)
    fwd_refused("unknown flag", flags=4, io=io_(obs_self=None), no_st=True)
    fwd_refused("observation pointer missing", io=io_(obs_self=None), no_st=True)
    fwd_refused("observation pointer missing", io=io_(obs_others=None), no_st=True)
    fwd_refused("misaligned observation", io=io_(obs_cylinders=0x1002), no_st=True)
    fwd_refused("negative stride", io=io_(cyl_stride=[1, -1, 1]), no_st=True)
    fwd_refused("state pointer", no_st=True, io=io_(value=None))
    fwd_refused("state pointer", st=st_(state_drones=None), io=io_(value=None))
    fwd_refused("state pointer", st=st_(cylinders=0x1001), io=io_(value=None))
    fwd_refused("negative stride", st=st_(drones_stride=[-1, 0]), io=io_(value=None))
    fwd_refused("value output", io=io_(value=None, action=None))
    fwd_refused("action / log_prob", io=io_(action=None), counter=None)
    fwd_refused("action / log_prob", io=io_(loc=0x1002), counter=None)
    fwd_refused("device call counter", counter=None)
    fwd_refused("misaligned eps", io=io_(eps=0x1002))
    # value-only: the observation is not looked at, the state and the value still are
    fwd_refused("state pointer", flags=abi.HNS_POLICY_VALUE_ONLY, io=io_(obs_self=None, obs_others=None, obs_cylinders=None), no_st=True)
    fwd_refused("value output", flags=abi.HNS_POLICY_VALUE_ONLY, io=io_(obs_self=None, obs_others=None, obs_cylinders=None, value=0x1002))
