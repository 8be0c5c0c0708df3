"""The centralised critic (critic_input: state) on the CPU: the golden fixture executed from the reference's own classes
(tests/golden/make_golden_policy_central.py), the two restatements (tests/central_reference.py, hns_amd.policy.torch_forward_central), the
CPU-tensor paths of CentralCriticDevicePolicy and update_critic_central under the fp64 gate, the refusal matrix and the checkpoint round trip.
DESIGN.md §7.20."""
import os

import numpy as np
import pytest
import torch

import central_reference as CR
import critic_update_reference as U
import policy_reference as R
from hns_amd import critic_train as CT
from hns_amd import policy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("a3k3d35", "a1k3d20", "a4k5d20")


@pytest.fixture(scope="module")
def gc():
    return np.load(os.path.join(ROOT, "tests", "golden", "g_policy_central.npz"))


def _t(d):
    return {k: torch.as_tensor(v) for k, v in d.items()}


def _actor(D, A, seed=3):
    return P.random_parameters(D, A, seed)[0]


def _obs(E, A, K, D, seed):
    obs, eps = R.random_obs(E, A, K, D, seed)
    return (torch.as_tensor(obs["state_self"]), torch.as_tensor(obs["state_others"]) if A > 1 else None, torch.as_tensor(obs["cylinders"]),
            torch.as_tensor(eps))


def test_fixture_is_no_larger_than_the_obs_critics():
    g = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(g, "g_policy_central.npz")) <= os.path.getsize(os.path.join(g, "g_policy.npz"))


@pytest.mark.parametrize("tag", CASES)
def test_restatements_meet_the_reference_fixture(gc, tag):
    """(A, K, D) = (3, 3, 35), (1, 3, 20), (4, 5, 20): central_reference in fp64 and fp32 and policy.torch_forward_central against the value
    the reference's Critic(centralized=True) computed, at test_policy_net.py's tolerance for g_policy.npz."""
    critic, sd, cyl, want = CR.golden_case(gc, tag)
    B, A, K, D = (int(x) for x in gc[f"{tag}:shape"])
    assert list(critic) == [n for n in P.CENTRAL_CRITIC_NAMES if n in critic] and len(critic) == 20 and want.shape == (B, A, 1)
    assert critic["v_out.weight"].shape == (A, 128) and critic["base.split_embed.embed.state_drones.weight"].shape == (128, D)
    for dtype in (torch.float64, torch.float32):
        np.testing.assert_allclose(CR.value_np(critic, sd, cyl, dtype), want, atol=1e-5, rtol=1e-5, err_msg=f"{tag} {dtype}")
    p = P.parse_parameters_central(_t(critic))[0]
    got = P.torch_forward_central(None, p, None, None, None, torch.as_tensor(sd), torch.as_tensor(cyl), value_only=True).value
    np.testing.assert_allclose(got.numpy(), want, atol=1e-5, rtol=1e-5, err_msg=f"{tag} (policy.py)")


def test_names_and_tensor_count():
    assert len(P.CENTRAL_CRITIC_NAMES) == 20 and not any("state_others" in k or "state_self" in k for k in P.CENTRAL_CRITIC_NAMES)
    assert set(P.CENTRAL_CRITIC_NAMES.values()) == set(P.CRITIC_NAMES.values()) - {"embed_others_w", "embed_others_b"}
    _, critic = P.random_parameters_central(35, 3, 0)
    assert list(critic) == list(P.CENTRAL_CRITIC_NAMES) or set(critic) == set(P.CENTRAL_CRITIC_NAMES)
    assert critic["v_out.weight"].shape == (3, 128) and critic["v_out.bias"].shape == (3,)


@pytest.mark.parametrize("shape", [(33, 3, 5, 35), (1, 3, 3, 20), (64, 2, 1, 20), (40, 7, 16, 96), (32, 1, 5, 20)])
def test_cpu_policy_passes_the_fp64_gate_and_keeps_the_actor(shape):
    """CentralCriticDevicePolicy on CPU tensors: value under the gate against central_reference; action, log_prob and loc are DevicePolicy's
    bits for the same actor and eps (the same torch statements); value_only sets value alone."""
    E, A, K, D = shape
    critic = CR.random_critic(D, A, 11 + A)
    sd, cyl = CR.random_state(E, A, K, D, 12)
    xs, xo, xc, eps = _obs(E, A, K, D, 13)
    actor = _actor(D, A)
    pol = P.CentralCriticDevicePolicy(actor, _t(critic))
    assert pol.needs_state and pol.num_agents == A and not P.DevicePolicy.needs_state
    out = pol.forward(xs, xo, xc, torch.as_tensor(sd), torch.as_tensor(cyl), eps=eps)
    assert out.value.shape == (E, A, 1)
    r64, r32 = CR.value_np(critic, sd, cyl, torch.float64), CR.value_np(critic, sd, cyl, torch.float32)
    assert CR.ratio(out.value.numpy(), r64, r32) <= CR.BAR
    ref = P.DevicePolicy(actor, P.random_parameters(D, A, 5)[1]).forward(xs, xo, xc, eps=eps)
    for n in ("action", "log_prob", "loc"):
        assert torch.equal(getattr(out, n), getattr(ref, n)), n
    vo = pol.forward(xs, xo, xc, torch.as_tensor(sd), torch.as_tensor(cyl), value_only=True)
    assert vo.action is None and vo.log_prob is None and vo.loc is None and torch.equal(vo.value, out.value)
    # the env's [E, A, K, 5] tensor: agent 0's rows; None: agent 0's rows of the observation's
    wide = torch.as_tensor(cyl).unsqueeze(1).repeat(1, A, 1, 1).contiguous()
    wide[:, 1:] += 1.0
    assert torch.equal(pol.forward(xs, xo, xc, torch.as_tensor(sd), wide, value_only=True).value, out.value)
    assert torch.equal(pol.forward(xs, xo, wide, torch.as_tensor(sd), value_only=True).value, out.value)


def test_one_agent_is_the_obs_critic_on_the_same_tensors():
    """A = 1: the state's tokens are the observation's (one drone row, then the cylinders), so torch_forward_central's value equals
    torch_forward's on the same 20 tensors with state_drones as obs_self."""
    E, K, D = 17, 5, 20
    actor, critic = P.random_parameters(D, 1, 21)
    xs, _, xc, _ = _obs(E, 1, K, D, 22)
    a, c = P.parse_parameters(actor, P.ACTOR_NAMES, "actor"), P.parse_parameters(critic, P.CRITIC_NAMES, "critic")
    want = P.torch_forward(a, c, xs, None, xc, value_only=True).value
    central = {k.replace("state_self", "state_drones"): v for k, v in critic.items()}
    cp, A = P.parse_parameters_central(central)
    got = P.torch_forward_central(a, cp, xs, None, xc, xs.squeeze(2), xc[:, 0], value_only=True).value
    assert A == 1 and torch.equal(got, want)


VARIANTS = {"huber": {}, "mse": {"loss": "mse"}, "far_returns": {}, "tie": {"clip_param": 100.0}}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", [(3, 5, 35, 33), (7, 16, 96, 9), (2, 1, 20, 1), (1, 5, 20, 40)])
def test_cpu_update_passes_the_fp64_gate(shape, variant):
    """update_critic_central's CPU-tensor path (value_loss_and_grad_central) against central_reference: the 20 gradients, the scalars and the
    values; far_returns: the clipped branch wins; tie: b_values 0 and a clip wider than every value."""
    A, K, D, S = shape
    critic = CR.random_critic(D, A, 100 + A + K)
    sd, cyl = CR.random_state(S, A, K, D, 101)
    far = variant == "far_returns"
    bv, ret = CR.targets(critic, sd, cyl, 102, ret_scale=40.0 if far else 1.0, shift=-0.5 if far else None)
    if variant == "tie":
        bv = np.zeros_like(bv)
    kw = VARIANTS[variant]
    r64 = CR.loss_and_grad(critic, sd, cyl, bv, ret, dtype=torch.float64, **kw)
    r32 = CR.loss_and_grad(critic, sd, cyl, bv, ret, dtype=torch.float32, **kw)
    if variant == "tie":
        assert r64["branch"] == 2 and r32["branch"] == 2
    elif far and S > 1:
        assert r64["branch"] == 1
    c = _t(critic)
    out = CT.value_loss_and_grad_central(c, torch.as_tensor(sd), torch.as_tensor(cyl), torch.as_tensor(bv), torch.as_tensor(ret), **kw)
    got = {"value_loss": float(out.value_loss), "explained_var": float(out.explained_var), "grad_norm": float(out.grad_norm),
           "values": out.values.numpy(), "grads": {k: v.grad.double().numpy() for k, v in c.items()}}
    if S * A == 1:                                             # var() of one return is NaN on both sides
        assert np.isnan(got["explained_var"]) and np.isnan(r64["explained_var"])
        got["explained_var"] = r64["explained_var"] = r32["explained_var"] = 0.0
    CR.gate_update(f"cpu-a{A}k{K}d{D}s{S}-{variant}", got, r64, r32, log=lambda *_: None)


def test_cpu_update_reads_an_index_and_the_rollouts_cylinders_in_place():
    """(3, 5, 35, 65) with a permuted index: the [N, T, A, K, 5] observation tensor gives what agent 0's rows as [N, T, K, 5] give; one
    ClippedAdam step follows clip_adam_np within fp32 rounding of the CPU path (torch's own Adam arithmetic)."""
    A, K, D, S = 3, 5, 35, 65
    critic = CR.random_critic(D, A, 131)
    sd, cyl = CR.random_state(S, A, K, D, 132)
    bv, ret = CR.targets(critic, sd, cyl, 133)
    index = np.random.default_rng(5).permutation(S)[:50]
    r64 = CR.loss_and_grad(critic, sd, cyl, bv, ret, index, dtype=torch.float64)
    r32 = CR.loss_and_grad(critic, sd, cyl, bv, ret, index, dtype=torch.float32)
    wide = np.repeat(cyl[:, None], A, axis=1)
    wide[:, 1:] += 1.0
    lay = lambda x: torch.as_tensor(x).reshape(5, 13, *x.shape[1:])
    for xc in (lay(cyl), lay(wide)):
        c = {k: torch.nn.Parameter(torch.tensor(v)) for k, v in critic.items()}      # (a copy: the step is in place)
        opt = CT.make_optimizer(c)
        assert len(opt.param_groups[0]["params"]) == 20
        out = CT.value_loss_and_grad_central(c, lay(sd), xc, lay(bv), lay(ret), torch.as_tensor(index))
        got = {"value_loss": float(out.value_loss), "explained_var": float(out.explained_var), "grad_norm": float(out.grad_norm),
               "values": out.values.numpy(), "grads": {k: v.grad.double().numpy() for k, v in c.items()}}
        CR.gate_update("cpu-index", got, r64, r32, log=lambda *_: None)
        info = CT.update_critic_central(c, lay(sd), xc, lay(bv), lay(ret), opt, index=torch.as_tensor(index))
        assert set(info) == {"value_loss", "critic_grad_norm", "explained_var"} and all(v.dim() == 0 for v in info.values())
        assert any(not np.array_equal(c[k].detach().numpy(), critic[k]) for k in c)


def _cfg(**kw):
    return {"share_actor": True, "critic_input": "state", **kw}


def test_refusal_matrix():
    """Each raises before anything is built, with the existing exception types; DevicePolicy and its subclasses keep refusing
    critic_input: state."""
    D, A = 20, 3
    actor, critic = P.random_parameters_central(D, A, 1)
    obs_critic = P.random_parameters(D, A, 1)[1]
    ok = P.CentralCriticDevicePolicy(actor, critic, cfg=_cfg())
    assert ok.num_agents == A and ok.self_dim == D
    E = P.PolicyConfigError
    with pytest.raises(E, match="critic_input"):
        P.CentralCriticDevicePolicy(actor, critic, cfg={"critic_input": "obs"})
    with pytest.raises(E, match="share_actor"):
        P.CentralCriticDevicePolicy(actor, critic, cfg=_cfg(share_actor=False))
    with pytest.raises(E, match="rnn"):
        P.CentralCriticDevicePolicy(actor, critic, cfg=_cfg(actor={"rnn": {"cls": "gru"}}))
    with pytest.raises(E, match="rnn"):
        P.CentralCriticDevicePolicy(actor, critic, cfg=_cfg(critic={"rnn": {"cls": "gru"}}))
    with pytest.raises(E, match="tanh"):
        P.CentralCriticDevicePolicy(actor, critic, cfg=_cfg(actor={"tanh": True}))
    with pytest.raises(E, match="leading agent dimension"):
        P.CentralCriticDevicePolicy(P.random_parameters_per_agent(D, A, 1)[0], critic)
    with pytest.raises(E, match="rnn"):
        P.CentralCriticDevicePolicy({**actor, **{"rnn." + k[4:]: v for k, v in P.random_rnn_parameters(1).items()}}, critic)
    with pytest.raises(E, match="rnn"):
        P.CentralCriticDevicePolicy(actor, {**critic, **P.random_rnn_parameters(1)})
    with pytest.raises(E, match="state_others"):
        P.CentralCriticDevicePolicy(actor, {**critic, "base.split_embed.embed.state_others.weight": torch.zeros(128, 3),
                                            "base.split_embed.embed.state_others.bias": torch.zeros(128)})
    with pytest.raises(E, match="state_self|state_others"):
        P.CentralCriticDevicePolicy(actor, obs_critic)                         # the obs critic's 22 tensors
    with pytest.raises(E, match="v_out"):
        P.CentralCriticDevicePolicy(actor, {**critic, "v_out.weight": critic["v_out.weight"][:1].clone(), "v_out.bias": critic["v_out.bias"][:1].clone()})
    with pytest.raises(E, match="v_out"):
        P.CentralCriticDevicePolicy(actor, {**critic, "v_out.weight": torch.zeros(8, 128), "v_out.bias": torch.zeros(8)})
    with pytest.raises(E, match="different widths"):
        P.CentralCriticDevicePolicy(actor, P.random_parameters_central(D + 1, A, 1)[1])
    # the existing classes: unchanged refusals
    with pytest.raises(E, match="centralised critic"):
        P.DevicePolicy(actor, obs_critic, cfg={"critic_input": "state"})
    with pytest.raises(E, match="does not have"):
        P.DevicePolicy(actor, critic)
    with pytest.raises(E, match="centralised critic"):
        P.PerAgentDevicePolicy(P.random_parameters_per_agent(D, A, 1)[0], obs_critic, cfg={"share_actor": False, "critic_input": "state"})
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
        P.CentralCriticDevicePolicy(*P.random_parameters_central(D, 2, 1)).forward(xs, xo, xc, sd)


def test_update_refusals():
    D, A, K, S = 20, 3, 5, 12
    critic = {k: torch.nn.Parameter(v) for k, v in P.random_parameters_central(D, A, 1)[1].items()}
    sd, cyl = (torch.as_tensor(x) for x in CR.random_state(S, A, K, D, 2))
    bv = ret = torch.zeros(S, A, 1)
    opt = CT.make_optimizer(critic, cfg=_cfg())
    with pytest.raises(P.PolicyConfigError, match="critic_input"):
        CT.make_optimizer(critic, cfg={"critic_input": "obs"})
    with pytest.raises(P.PolicyConfigError, match="centralised critic"):
        CT.make_optimizer(P.random_parameters(D, A, 1)[1], cfg=_cfg())         # the obs critic keeps refusing critic_input: state
    with pytest.raises(TypeError, match="ClippedAdam"):
        CT.update_critic_central(critic, sd, cyl, bv, ret, torch.optim.Adam(critic.values()))
    with pytest.raises(P.PolicyConfigError, match="critic_input"):
        CT.update_critic_central(critic, sd, cyl, bv, ret, opt, cfg={"critic_input": "obs"})
    with pytest.raises(P.PolicyConfigError, match="rnn"):
        CT.update_critic_central(critic, sd, cyl, bv, ret, opt, cfg=_cfg(critic={"rnn": {"cls": "gru"}}))
    with pytest.raises(ValueError, match="v_out has 3 rows"):
        CT.value_loss_and_grad_central(critic, sd[:, :2], cyl, bv, ret)
    with pytest.raises(ValueError, match="cylinders"):
        CT.value_loss_and_grad_central(critic, sd, cyl[..., :4], bv, ret)
    with pytest.raises(ValueError, match="b_values"):
        CT.value_loss_and_grad_central(critic, sd, cyl, bv[:, :2], ret)
    with pytest.raises(TypeError, match="int64"):
        CT.value_loss_and_grad_central(critic, sd, cyl, bv, ret, index=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(IndexError):
        CT.value_loss_and_grad_central(critic, sd, cyl, bv, ret, index=torch.tensor([0, S]))
    with pytest.raises(ValueError, match="loss"):
        CT.value_loss_and_grad_central(critic, sd, cyl, bv, ret, loss="l1")
    with pytest.raises(P.PolicyConfigError):
        CT.value_loss_and_grad_central(P.random_parameters(D, A, 1)[1], sd, cyl, bv, ret)
    assert all(v.grad is None for v in critic.values())


def test_checkpoint_round_trip_under_the_reference_names(tmp_path):
    D, A = 20, 3
    actor, critic = P.random_parameters_central(D, A, 4)
    ck = {"actor_params": {"module." + k: v for k, v in actor.items()}, "critic": {"module." + k: v for k, v in critic.items()}}
    assert "module.base.split_embed.embed.state_drones.weight" in ck["critic"] and ck["critic"]["module.v_out.weight"].shape == (A, 128)
    path = tmp_path / "policy.pt"
    torch.save(ck, path)
    pol = P.CentralCriticDevicePolicy.from_checkpoint(str(path), cfg=_cfg())
    for k, f in P.CENTRAL_CRITIC_NAMES.items():
        assert torch.equal(pol.critic_p[f], critic[k]), k
    xs, xo, xc, eps = _obs(5, A, 4, D, 6)
    sd = torch.randn(5, A, D, generator=torch.Generator().manual_seed(1))
    a = pol.forward(xs, xo, xc, sd, eps=eps)
    b = P.CentralCriticDevicePolicy(actor, critic).forward(xs, xo, xc, sd, eps=eps)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(P.PolicyConfigError):
        P.DevicePolicy.from_checkpoint(str(path))


def test_call_and_value_read_the_state_group():
    D, A, E, K = 20, 3, 6, 4
    pol = P.CentralCriticDevicePolicy(*P.random_parameters_central(D, A, 8))
    xs, xo, xc, _ = _obs(E, A, K, D, 9)
    sd = torch.randn(E, A, D, generator=torch.Generator().manual_seed(2))
    td = {("agents", "observation"): {"state_self": xs, "state_others": xo, "cylinders": xc}, ("agents", "state"): {"state_drones": sd, "cylinders": xc}}
    want = pol.forward(xs, xo, xc, sd, xc[:, 0].contiguous(), value_only=True).value
    assert torch.equal(pol.value(td), want)
    out = pol(dict(td), deterministic=True)
    assert torch.equal(out["state_value"], want) and out[("agents", "action")].shape == (E, A, 4) and out["drone.action_logp"].shape == (E, A, 1)
    assert torch.equal(pol.act(xs, xo, xc), out[("agents", "action")])
