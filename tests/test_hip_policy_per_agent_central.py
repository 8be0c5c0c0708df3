"""Per-agent actors beside the centralised critic on an MI355X: hns_policy_pack_central_agents and hns_policy_central_forward_agents through
hns_amd.policy.PerAgentCentralCriticDevicePolicy.  DESIGN.md §7.21.

The entry is the join of two pinned paths, so its yardsticks are bit identities: for every row (e, a), action, log_prob and loc are
PerAgentDevicePolicy's (hns_policy_forward_agents) for the same stacked actor, with eps and with the same (seed, counter); value is
CentralCriticDevicePolicy's (hns_policy_central_forward) for the same critic and state, and under the project's fp64 gate
(tests/central_reference.py, BAR 8).

Shapes (E, A, K, D): (33, 3, 5, 35) two tiles per range, the second with one live env; (1, 3, 3, 20) a single env; (64, 2, 1, 20) exactly two
full tiles; (40, 7, 16, 96) every limit; (32, 1, 5, 20) one agent; (97, 3, 5, 35) past three tiles."""
import ctypes as C

import numpy as np
import pytest
import torch

import central_reference as CR
import policy_reference as R
from hns_amd import abi
from hns_amd import policy as P

pytestmark = pytest.mark.gpu

SHAPES = [(33, 3, 5, 35), (1, 3, 3, 20), (64, 2, 1, 20), (40, 7, 16, 96), (32, 1, 5, 20), (97, 3, 5, 35)]
OUTS = ("action", "log_prob", "loc")
RATIOS = {}


def _cuda(d):
    return {k: torch.as_tensor(v).cuda().contiguous() for k, v in d.items()}


def _case(shape, seed=0):
    """The stacked actor (agents that differ in every tensor, log_std included), the obs critic and a shared actor for the two reference
    classes, the centralised critic, observations, eps and the state — all built once per shape and never written."""
    E, A, K, D = shape
    stacked, obs_critic = P.random_parameters_per_agent(D, A, 40 + seed + A)
    g = torch.Generator().manual_seed(41 + seed)
    stacked = {k: v + torch.randn(v.shape, generator=g) * (0.3 if k.endswith("log_std") else 0.05) for k, v in stacked.items()}
    stacked["act_dist.fc_mean.weight"] = stacked["act_dist.fc_mean.weight"] * 30.0
    shared_actor = P.random_parameters(D, A, 43 + seed)[0]
    critic = CR.random_critic(D, A, 50 + seed + A)
    obs, eps = R.random_obs(E, A, K, D, 60 + seed)
    sd, cyl = CR.random_state(E, A, K, D, 70 + seed)
    d = lambda x: torch.as_tensor(x).cuda()                       # noqa: E731
    xs, xo, xc = d(obs["state_self"]), (d(obs["state_others"]) if A > 1 else None), d(obs["cylinders"])
    return {"stacked": _cuda(stacked), "obs_critic": _cuda(obs_critic), "shared_actor": _cuda(shared_actor), "critic": _cuda(critic),
            "critic_np": critic, "obs": (xs, xo, xc), "eps": d(eps), "sd": d(sd), "cyl": d(cyl), "state_np": (sd, cyl)}


@pytest.fixture(scope="module")
def cases():
    return {s: _case(s) for s in SHAPES}


def _policies(c, seed=77):
    new = P.PerAgentCentralCriticDevicePolicy(c["stacked"], c["critic"], cfg={"share_actor": False, "critic_input": "state"}, seed=seed)
    agents = P.PerAgentDevicePolicy(c["stacked"], c["obs_critic"], seed=seed)
    central = P.CentralCriticDevicePolicy(c["shared_actor"], c["critic"], seed=seed)
    return new, agents, central


@pytest.mark.parametrize("shape", SHAPES)
def test_actor_rows_and_value_are_the_two_pinned_paths_bits(cases, shape):
    E, A, K, D = shape
    c = cases[shape]
    obs, eps, sd, cyl = c["obs"], c["eps"], c["sd"], c["cyl"]
    pol, agents, central = _policies(c)
    out, want_a, want_c = pol.forward(*obs, sd, cyl, eps=eps), agents.forward(*obs, eps=eps), central.forward(*obs, sd, cyl, eps=eps)
    for n in OUTS:
        assert torch.equal(getattr(out, n), getattr(want_a, n)), f"{n} (eps)"
    assert out.value.shape == (E, A, 1) and torch.equal(out.value, want_c.value)
    sd_np, cyl_np = c["state_np"]
    x = CR.ratio(out.value.cpu().numpy(), CR.value_np(c["critic_np"], sd_np, cyl_np, torch.float64), CR.value_np(c["critic_np"], sd_np, cyl_np, torch.float32))
    RATIOS[shape] = x
    print(f"  per-agent central value {shape}: ratio {x:.2f}")
    assert x <= CR.BAR, f"value: ratio {x:.2f}"
    # the same seed and call counter: the same Philox noise per row
    a, b = pol.forward(*obs, sd, cyl), agents.forward(*obs)
    for n in OUTS:
        assert torch.equal(getattr(a, n), getattr(b, n)), f"{n} (seed, counter)"
    assert int(pol.counter) == int(agents.counter) == 1 and not torch.equal(a.action, out.action)
    assert torch.equal(a.value, out.value)
    # the mode: action = loc = act = PerAgentDevicePolicy.act; the counter stays
    det = pol.forward(*obs, sd, cyl, deterministic=True)
    assert torch.equal(det.action, det.loc) and torch.equal(det.loc, out.loc)
    assert torch.equal(det.action, pol.act(*obs)) and torch.equal(det.action, agents.act(*obs))
    assert torch.equal(det.value, out.value) and int(pol.counter) == 1
    assert torch.equal(pol.scale, agents.scale) and tuple(pol.scale.shape) == (A, 4)
    # two calls in a row
    again = pol.forward(*obs, sd, cyl, eps=eps)
    assert all(torch.equal(x, y) for x, y in zip(out, again))


def _raw(pol, obs, sd, cyl, flags, action, loc, logp, value, eps=None, null_obs=False):
    """hns_policy_central_forward_agents on the caller's output buffers; null_obs: the three observation pointers NULL."""
    xs, xo, xc = pol._validate(*obs)
    pol.refresh()
    xs, xo, xc, io = pol._io(xs, xo, xc)
    if null_obs:
        io.obs_self = io.obs_others = io.obs_cylinders = None
    io.action, io.loc, io.log_prob, io.value = action.data_ptr(), loc.data_ptr(), logp.data_ptr(), value.data_ptr()
    io.eps = eps.data_ptr() if eps is not None else None
    st = abi.HnsPolicyState()
    st.state_drones, st.cylinders = sd.data_ptr(), cyl.data_ptr()
    st.drones_stride[:] = [sd.stride(0), sd.stride(1)]
    st.cyl_stride[:] = [cyl.stride(0), cyl.stride(1)]
    E, A = xs.shape[:2]
    return pol._lib.hns_policy_central_forward_agents(pol.packed.data_ptr(), pol.self_dim, E, A, xc.shape[2], C.byref(io), C.byref(st), flags, pol.seed,
                                                      pol.counter.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("shape", SHAPES)
def test_value_only_and_guard_rows(cases, shape):
    """HNS_POLICY_VALUE_ONLY launches the critic's range alone, with NULL observations: pre-filled action, log_prob and loc keep every bit,
    the counter stays, and the guard rows around every output (in front of row 0 and behind row E A) keep their sentinel — in a full call too."""
    E, A, K, D = shape
    c = cases[shape]
    obs, eps, sd, cyl = c["obs"], c["eps"], c["sd"], c["cyl"]
    pol = _policies(c)[0]
    want = pol.forward(*obs, sd, cyl, eps=eps)
    G, n = 64, E * A
    full = [torch.full((G + n + G, w), -7.5, device="cuda") for w in (4, 4, 1, 1)]
    bufs = [t[G:] for t in full]
    guards_kept = lambda: all(bool((t[:G] == -7.5).all()) and bool((t[G + n:] == -7.5).all()) for t in full)       # noqa: E731
    assert _raw(pol, obs, sd, cyl, abi.HNS_POLICY_VALUE_ONLY, *bufs, null_obs=True) == abi.HNS_OK
    torch.cuda.synchronize()
    action, loc, logp, value = (t[G:G + n] for t in full)
    assert all(bool((t == -7.5).all()) for t in (action, loc, logp)) and guards_kept() and int(pol.counter) == 0
    assert torch.equal(value.view(E, A, 1), want.value)
    assert torch.equal(pol.forward(*obs, sd, cyl, value_only=True).value, want.value)
    assert _raw(pol, obs, sd, cyl, 0, *bufs, eps=eps.contiguous()) == abi.HNS_OK
    torch.cuda.synchronize()
    for t, w in ((action, want.action), (loc, want.loc), (logp, want.log_prob), (value, want.value)):
        assert torch.equal(t.view(w.shape), w)
    assert guards_kept() and int(pol.counter) == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_strided_state_and_the_envs_cylinders_read_in_place(cases, shape):
    E, A, K, D = shape
    c = cases[shape]
    obs, sd, cyl = c["obs"], c["sd"], c["cyl"]
    pol = _policies(c)[0]
    want = pol.forward(*obs, sd, cyl, eps=c["eps"])
    # the env's [E, A, K, 5] tensor: agent 0's rows in place (the other agents' rows hold something else)
    wide = cyl.unsqueeze(1).repeat(1, A, 1, 1).contiguous()
    wide[:, 1:] += 1.0
    # state_drones as a strided view: every second row of a taller tensor, the last axis cut from a wider one
    tall = torch.full((E, 2 * A, D + 3), 9.0, device="cuda")
    tall[:, ::2, :D] = sd
    view = tall[:, ::2, :D]
    assert not view.is_contiguous() and view.stride(-1) == 1
    got = pol.forward(*obs, view, wide, eps=c["eps"])
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert torch.equal(pol.forward(obs[0], obs[1], wide, sd, value_only=True).value, want.value)          # state_cylinders=None


@pytest.mark.parametrize("shape", SHAPES)
def test_one_single_stream_graph_replay_has_the_eager_bits(cases, shape):
    c = cases[shape]
    obs, eps, sd, cyl = c["obs"], c["eps"], c["sd"], c["cyl"]
    pol = _policies(c)[0]
    eager = pol.forward(*obs, sd, cyl, eps=eps)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = pol.forward(*obs, sd, cyl, eps=eps)
    for t in g:
        t.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(eager, g))


def test_agents_rows_come_from_their_own_images(cases):
    """Distinctness: the actors differ per agent, so agent a's rows differ from what agent b's slice gives them — a tile that read another
    agent's image would show in the identities above."""
    shape = (33, 3, 5, 35)
    c = cases[shape]
    obs, eps, sd, cyl = c["obs"], c["eps"], c["sd"], c["cyl"]
    out = _policies(c)[0].forward(*obs, sd, cyl, eps=eps)
    for b in range(shape[1]):
        shared = P.CentralCriticDevicePolicy({k: v[b] for k, v in c["stacked"].items()}, c["critic"]).forward(*obs, sd, cyl, eps=eps)
        for a in range(shape[1]):
            for n in OUTS:
                assert torch.equal(getattr(out, n)[:, a], getattr(shared, n)[:, a]) == (a == b), (n, a, b)
        assert torch.equal(out.value, shared.value)


@pytest.mark.parametrize("shape", [(33, 3, 5, 35), (40, 7, 16, 96), (32, 1, 5, 20)])
def test_image_is_the_agents_images_then_the_central_tail(cases, shape):
    E, A, K, D = shape
    c = cases[shape]
    pol, agents, central = _policies(c)
    for p in (pol, agents, central):
        p.refresh()
    torch.cuda.synchronize()
    net = pol._lib.hns_policy_packed_bytes(D) // 2                # one network's image, in bytes
    assert pol.packed.numel() == pol._lib.hns_policy_packed_central_agents_bytes(D, A) == A * net + central.packed.numel() - net
    assert torch.equal(pol.packed[:A * net], agents.packed[:A * net])
    assert torch.equal(pol.packed[A * net:], central.packed[net:])
    # a critic with a state_others embedding is refused by the C entry too
    bad = pol._net(pol.critic_p)
    bad.embed_others_w = bad.embed_others_b = pol.critic_p["ln_w"].data_ptr()
    rc = pol._lib.hns_policy_pack_central_agents(C.byref(pol._net(pol.actor_p)), C.byref(bad), D, A, pol.packed.data_ptr(), None)
    assert rc != abi.HNS_OK and b"state_others" in pol._lib.hns_last_error()


def test_refresh_follows_an_optimiser_step(cases):
    shape = (33, 3, 5, 35)
    c = cases[shape]
    obs, eps, sd, cyl = c["obs"], c["eps"], c["sd"], c["cyl"]
    actor = {k: torch.nn.Parameter(v.clone()) for k, v in c["stacked"].items()}
    critic = {k: torch.nn.Parameter(v.clone()) for k, v in c["critic"].items()}
    pol = P.PerAgentCentralCriticDevicePolicy(actor, critic)
    before = [t.clone() for t in pol.forward(*obs, sd, cyl, eps=eps)]
    opt = torch.optim.SGD([*actor.values(), *critic.values()], lr=0.05)
    for v in (*actor.values(), *critic.values()):
        v.grad = torch.ones_like(v)
    opt.step()
    after = pol.forward(*obs, sd, cyl, eps=eps)
    assert not torch.equal(before[0], after.action) and not torch.equal(before[2], after.value)
    fresh = P.PerAgentCentralCriticDevicePolicy({k: v.detach().clone() for k, v in actor.items()}, {k: v.detach().clone() for k, v in critic.items()})
    assert all(torch.equal(x, y) for x, y in zip(after, fresh.forward(*obs, sd, cyl, eps=eps)))


def test_evaluator_has_the_per_agent_policys_bits():
    """An 8-step DeviceEvaluator.evaluate() over the new policy against one over a PerAgentDevicePolicy with the same stacked actor:
    evaluator.py needs no change (it runs `act`, which this image serves through hns_policy_act_agents)."""
    from hns_amd import config
    from hns_amd.env import HideAndSeek
    from hns_amd.evaluator import DeviceEvaluator
    cfg = config.make_cfg({"num_agents": 3, "env": {"num_envs": 8, "max_episode_length": 8}},
                          algo={"use_TP_net": 0, "critic_input": "state", "share_actor": False})
    env = HideAndSeek(cfg, headless=True)
    try:
        env.set_seed(3)
        D = abi.self_dim(env.num_targets)
        stacked, obs_critic = P.random_parameters_per_agent(D, 3, 9)
        stacked["act_dist.fc_mean.weight"] = stacked["act_dist.fc_mean.weight"] * 30.0    # actions of order 0.3: the drones move
        critic = P.random_parameters_central(D, 3, 9)[1]
        new = P.PerAgentCentralCriticDevicePolicy(stacked, critic, device=env.device, seed=1)
        old = P.PerAgentDevicePolicy(stacked, obs_critic, device=env.device, seed=1)
        a, b = DeviceEvaluator(env, new).evaluate(seed=5), DeviceEvaluator(env, old).evaluate(seed=5)
        assert list(a) == list(b) and len(a) > 3
        x, y = (np.array([float(d[k]) for k in a], np.float32) for d in (a, b))
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    finally:
        env.close()


def test_report_ratios():
    print("per-agent central value gate ratios:", {k: round(v, 2) for k, v in RATIOS.items()})
