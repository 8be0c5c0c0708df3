"""The centralised critic's forward pass on the device (hns_policy_pack_central, hns_policy_central_forward through
hns_amd.policy.CentralCriticDevicePolicy) on an MI355X.  DESIGN.md §7.20.

Shapes (E, A, K, D): (33, 3, 5, 35) — two critic tiles, the second with one live env, beside four actor tiles —, one env, two agents with one
cylinder, the limits A = 7 / K = 16 / D = 96, and one agent.  `value` is held to the project's fp64 gate (tests/central_reference.py, BAR 8);
action, log_prob and loc to DevicePolicy's bits; with one agent value too."""
import ctypes as C

import numpy as np
import pytest
import torch

import central_reference as CR
import policy_reference as R
from hns_amd import abi
from hns_amd import policy as P

pytestmark = pytest.mark.gpu

SHAPES = [(33, 3, 5, 35), (1, 3, 3, 20), (64, 2, 1, 20), (40, 7, 16, 96), (32, 1, 5, 20)]
RATIOS = {}


def _cuda(d):
    return {k: torch.as_tensor(v).cuda() for k, v in d.items()}


def _case(shape, seed=0):
    E, A, K, D = shape
    actor, obs_critic = R.random_net(D, A, 40 + seed + A, log_std=R.LOG_STD)
    critic = CR.random_critic(D, A, 50 + seed + A)
    obs, eps = R.random_obs(E, A, K, D, 60 + seed)
    sd, cyl = CR.random_state(E, A, K, D, 70 + seed)
    d = lambda x: torch.as_tensor(x).cuda()
    xs, xo, xc = d(obs["state_self"]), (d(obs["state_others"]) if A > 1 else None), d(obs["cylinders"])
    return actor, obs_critic, critic, (xs, xo, xc), d(eps), d(sd), d(cyl), (sd, cyl)


@pytest.fixture(scope="module")
def cases():
    return {s: _case(s) for s in SHAPES}


@pytest.mark.parametrize("shape", SHAPES)
def test_value_passes_the_fp64_gate_and_the_actor_keeps_its_bits(cases, shape):
    E, A, K, D = shape
    actor, obs_critic, critic, obs, eps, sd, cyl, (sd_np, cyl_np) = cases[shape]
    pol = P.CentralCriticDevicePolicy(_cuda(actor), _cuda(critic), seed=77)
    ref = P.DevicePolicy(_cuda(actor), _cuda(obs_critic), seed=77)
    out = pol.forward(*obs, sd, cyl, eps=eps)
    want = ref.forward(*obs, eps=eps)
    assert out.value.shape == (E, A, 1)
    x = CR.ratio(out.value.cpu().numpy(), CR.value_np(critic, sd_np, cyl_np, torch.float64), CR.value_np(critic, sd_np, cyl_np, torch.float32))
    RATIOS[shape] = x
    print(f"  central value {shape}: ratio {x:.2f}")
    assert x <= CR.BAR, f"value: ratio {x:.2f}"
    for n in ("action", "log_prob", "loc"):
        assert torch.equal(getattr(out, n), getattr(want, n)), f"{n} (eps)"
    # the same seed and call counter: the same Philox noise per row, whatever the critic
    a, b = pol.forward(*obs, sd, cyl), ref.forward(*obs)
    for n in ("action", "log_prob", "loc"):
        assert torch.equal(getattr(a, n), getattr(b, n)), f"{n} (seed, counter)"
    assert int(pol.counter) == int(ref.counter) == 1 and not torch.equal(a.action, out.action)
    assert torch.equal(a.value, out.value)
    det = pol.forward(*obs, sd, cyl, deterministic=True)
    assert torch.equal(det.action, det.loc) and torch.equal(det.action, pol.act(*obs)) and torch.equal(det.action, ref.act(*obs))
    assert int(pol.counter) == 1


def test_one_agent_value_is_the_obs_critics_bit_for_bit(cases):
    """A = 1: the state's tokens are the observation's, so with the same 20 tensors as DevicePolicy's critic and state_drones as its obs_self
    the two kernels run the same statements on the same numbers."""
    E, A, K, D = shape = (32, 1, 5, 20)
    actor, _, critic, obs, eps, sd, cyl, _ = cases[shape]
    as_obs = {k.replace("state_drones", "state_self"): v for k, v in critic.items()}
    want = P.DevicePolicy(_cuda(actor), _cuda(as_obs)).forward(sd.unsqueeze(2), None, cyl.unsqueeze(1), value_only=True).value
    got = P.CentralCriticDevicePolicy(_cuda(actor), _cuda(critic)).forward(*obs, sd, cyl, value_only=True).value
    assert torch.equal(got, want)


@pytest.mark.parametrize("shape", [(33, 3, 5, 35), (40, 7, 16, 96)])
def test_strided_state_reads_the_same_rows(cases, shape):
    E, A, K, D = shape
    actor, _, critic, obs, eps, sd, cyl, _ = cases[shape]
    pol = P.CentralCriticDevicePolicy(_cuda(actor), _cuda(critic))
    want = pol.forward(*obs, sd, cyl, value_only=True).value
    # the env's [E, A, K, 5] observation tensor: agent 0's rows in place (the other agents' rows hold something else)
    wide = cyl.unsqueeze(1).repeat(1, A, 1, 1).contiguous()
    wide[:, 1:] += 1.0
    assert torch.equal(pol.forward(*obs, sd, wide, value_only=True).value, want)
    assert torch.equal(pol.forward(obs[0], obs[1], wide, sd, value_only=True).value, want)          # state_cylinders=None
    assert torch.equal(pol.forward(*obs, sd, wide[:, 0].contiguous(), value_only=True).value, want)
    # state_drones as a strided view: every second row of a taller tensor, the last axis cut from a wider one
    tall = torch.full((E, 2 * A, D + 3), 9.0, device="cuda")
    tall[:, ::2, :D] = sd
    view = tall[:, ::2, :D]
    assert not view.is_contiguous() and view.stride(-1) == 1
    assert torch.equal(pol.forward(*obs, view, cyl, value_only=True).value, want)


def _raw(pol, obs, sd, cyl, flags, action, loc, logp, value, eps=None):
    """hns_policy_central_forward on the caller's output buffers."""
    xs, xo, xc = pol._validate(*obs)
    pol.refresh()
    xs, xo, xc, io = pol._io(xs, xo, xc)
    io.action, io.loc, io.log_prob, io.value = action.data_ptr(), loc.data_ptr(), logp.data_ptr(), value.data_ptr()
    io.eps = eps.data_ptr() if eps is not None else None
    st = abi.HnsPolicyState()
    st.state_drones, st.cylinders = sd.data_ptr(), cyl.data_ptr()
    st.drones_stride[:] = [sd.stride(0), sd.stride(1)]
    st.cyl_stride[:] = [cyl.stride(0), cyl.stride(1)]
    E, A = xs.shape[:2]
    rc = pol._lib.hns_policy_central_forward(pol.packed.data_ptr(), pol.self_dim, E, A, xc.shape[2], C.byref(io), C.byref(st), flags, pol.seed,
                                             pol.counter.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc


def test_value_only_and_guard_rows(cases):
    """HNS_POLICY_VALUE_ONLY launches the critic workgroups alone: pre-filled action, log_prob and loc keep every bit, and the rows behind
    value's E A keep their sentinel (so do those behind the actor's outputs in a full call)."""
    E, A, K, D = shape = (33, 3, 5, 35)
    actor, _, critic, obs, eps, sd, cyl, _ = cases[shape]
    pol = P.CentralCriticDevicePolicy(_cuda(actor), _cuda(critic))
    want = pol.forward(*obs, sd, cyl, eps=eps)
    G = 64
    bufs = [torch.full((E * A + G, w), -7.5, device="cuda") for w in (4, 4, 1, 1)]
    assert _raw(pol, obs, sd, cyl, abi.HNS_POLICY_VALUE_ONLY, *bufs) == abi.HNS_OK
    torch.cuda.synchronize()
    action, loc, logp, value = bufs
    assert all(bool((t == -7.5).all()) for t in (action, loc, logp)) and bool((value[E * A:] == -7.5).all())
    assert torch.equal(value[:E * A].view(E, A, 1), want.value)
    assert _raw(pol, obs, sd, cyl, 0, *bufs, eps=eps.contiguous()) == abi.HNS_OK
    torch.cuda.synchronize()
    for t, w in ((action, want.action), (loc, want.loc), (logp, want.log_prob), (value, want.value)):
        assert bool((t[E * A:] == -7.5).all()) and torch.equal(t[:E * A].view(w.shape), w)
    # the C entry's refusals come before any launch
    lib = pol._lib
    assert _raw(pol, obs, sd, cyl, 4, *bufs) != abi.HNS_OK and b"flag" in lib.hns_last_error()
    io = abi.HnsPolicyIo()
    assert lib.hns_policy_central_forward(pol.packed.data_ptr(), D, E, A, K, C.byref(io), None, 2, 0, None, None) != abi.HNS_OK
    assert lib.hns_policy_packed_central_bytes(D, 8) == 0 and lib.hns_policy_packed_central_bytes(97, 3) == 0
    assert lib.hns_policy_packed_central_bytes(D, A) > lib.hns_policy_packed_bytes(D) // 2


def test_pack_writes_the_shared_actors_image_byte_for_byte(cases):
    E, A, K, D = shape = (33, 3, 5, 35)
    actor, obs_critic, critic, *_ = cases[shape]
    pol = P.CentralCriticDevicePolicy(_cuda(actor), _cuda(critic))
    ref = P.DevicePolicy(_cuda(actor), _cuda(obs_critic))
    pol.refresh(), ref.refresh()
    half = ref.packed.numel() // 2
    assert torch.equal(pol.packed[:half], ref.packed[:half])
    assert torch.equal(pol.scale, ref.scale)
    # a critic with a state_others embedding is refused by the C entry too
    c = pol._net(pol.critic_p)
    c.embed_others_w = c.embed_others_b = pol.critic_p["ln_w"].data_ptr()
    rc = pol._lib.hns_policy_pack_central(C.byref(pol._net(pol.actor_p)), C.byref(c), D, A, pol.packed.data_ptr(), None)
    assert rc != abi.HNS_OK and b"state_others" in pol._lib.hns_last_error()


def test_same_bits_across_calls_and_one_graph_replay(cases):
    E, A, K, D = shape = (33, 3, 5, 35)
    actor, _, critic, obs, eps, sd, cyl, _ = cases[shape]
    pol = P.CentralCriticDevicePolicy(_cuda(actor), _cuda(critic))
    a, b = pol.forward(*obs, sd, cyl, eps=eps), pol.forward(*obs, sd, cyl, eps=eps)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
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
    assert all(torch.equal(x, y) for x, y in zip(a, g))


def test_refresh_follows_an_optimiser_step(cases):
    E, A, K, D = shape = (33, 3, 5, 35)
    actor, _, critic, obs, eps, sd, cyl, (sd_np, cyl_np) = cases[shape]
    dev = {k: torch.nn.Parameter(v) for k, v in _cuda(critic).items()}
    pol = P.CentralCriticDevicePolicy(_cuda(actor), dev)
    before = pol.forward(*obs, sd, cyl, value_only=True).value.clone()
    opt = torch.optim.SGD(dev.values(), lr=0.05)
    for v in dev.values():
        v.grad = torch.ones_like(v)
    opt.step()
    after = pol.forward(*obs, sd, cyl, value_only=True).value
    assert not torch.equal(before, after)
    new = {k: v.detach().cpu().numpy() for k, v in dev.items()}
    x = CR.ratio(after.cpu().numpy(), CR.value_np(new, sd_np, cyl_np, torch.float64), CR.value_np(new, sd_np, cyl_np, torch.float32))
    assert x <= CR.BAR, f"value after the step: ratio {x:.2f}"


def test_evaluator_is_unchanged_by_the_critic():
    """DeviceEvaluator runs `act` alone: with the new policy (on an env that writes state_drones) it gives bit for bit what a DevicePolicy
    over the same actor gives — evaluator.py needs no change."""
    from hns_amd import config
    from hns_amd.env import HideAndSeek
    from hns_amd.evaluator import DeviceEvaluator
    cfg = config.make_cfg({"num_agents": 3, "env": {"num_envs": 8, "max_episode_length": 6}}, algo={"use_TP_net": 0, "critic_input": "state"})
    env = HideAndSeek(cfg, headless=True)
    env.set_seed(3)
    D = abi.self_dim(env.num_targets)
    actor, critic = P.random_parameters_central(D, 3, 9)
    actor["act_dist.fc_mean.weight"] = actor["act_dist.fc_mean.weight"] * 30.0    # actions of order 0.3: the drones move
    new = P.CentralCriticDevicePolicy(actor, critic, device=env.device, seed=1)
    old = P.DevicePolicy(actor, P.random_parameters(D, 3, 9)[1], device=env.device, seed=1)
    a, b = DeviceEvaluator(env, new).evaluate(seed=5), DeviceEvaluator(env, old).evaluate(seed=5)
    assert list(a) == list(b) and len(a) > 3
    x, y = (np.array([float(d[k]) for k in a], np.float32) for d in (a, b))
    assert np.array_equal(x.view(np.int32), y.view(np.int32))


def test_report_ratios():
    print("central value gate ratios:", {k: round(v, 2) for k, v in RATIOS.items()})
