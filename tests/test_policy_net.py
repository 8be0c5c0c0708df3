"""The MAPPO policy's forward pass (hns_amd.policy), CPU side: the restatements against the reference's own networks (g_policy.npz, written by
tests/golden/make_golden_policy.py), parameter parsing from live objects and checkpoints, refusals, and the library's new symbols."""
import ctypes
import os

import numpy as np
import pytest
import torch

import policy_reference as R
from hns_amd import abi
from hns_amd import policy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["a3k5d35", "a3k8d20", "a1k5d20", "a6k16d24"]


@pytest.fixture(scope="module")
def gp():
    return np.load(os.path.join(ROOT, "tests", "golden", "g_policy.npz"))


def _obs_t(obs):
    return (torch.from_numpy(obs["state_self"]), torch.from_numpy(obs["state_others"]) if "state_others" in obs else None,
            torch.from_numpy(obs["cylinders"]))


@pytest.mark.parametrize("tag", CASES)
def test_restatements_match_the_reference_networks(gp, tag):
    actor, critic, obs, eps, exp = R.golden_case(gp, tag)
    for dtype in (torch.float32, torch.float64):
        loc, _, action, logp, value = R.forward(actor, critic, obs, eps, dtype=dtype)
        for name, got in (("loc", loc), ("action", action), ("log_prob", logp), ("value", value)):
            np.testing.assert_allclose(got.double().numpy(), exp[name], atol=1e-5, rtol=1e-5, err_msg=f"{tag} {name} {dtype}")
    # the product's CPU path (torch statements, F.multi_head_attention_forward)
    pol = P.DevicePolicy({k: torch.from_numpy(v) for k, v in actor.items()}, {k: torch.from_numpy(v) for k, v in critic.items()})
    out = pol.forward(*_obs_t(obs), eps=torch.from_numpy(eps))
    for name in ("loc", "action", "log_prob", "value"):
        np.testing.assert_allclose(getattr(out, name).numpy(), exp[name], atol=1e-5, rtol=1e-5, err_msg=f"{tag} {name} (policy.py)")
    det = pol.forward(*_obs_t(obs), deterministic=True)
    np.testing.assert_allclose(det.action.numpy(), exp["mode"], atol=1e-5, rtol=1e-5)
    assert torch.equal(det.action, det.loc)
    np.testing.assert_allclose(pol.forward(*_obs_t(obs), value_only=True).value.numpy(), exp["value"], atol=1e-5, rtol=1e-5)


class FakeTD:
    """TensorDictParams-like: nested keys, flatten_keys(sep) and items()."""

    def __init__(self, flat):
        self.flat = flat

    def flatten_keys(self, sep="."):
        return dict(self.flat)

    def items(self):
        return self.flat.items()


def _golden_params(gp, tag):
    actor, critic, _, _, _ = R.golden_case(gp, tag)
    return {k: torch.from_numpy(v.copy()) for k, v in actor.items()}, {k: torch.from_numpy(v.copy()) for k, v in critic.items()}


def test_names_with_and_without_the_module_prefix(gp):
    actor, critic = _golden_params(gp, "a3k5d35")
    plain = P.DevicePolicy(actor, critic)
    pref = P.DevicePolicy(FakeTD({"module." + k: v for k, v in actor.items()}), {"module." + k: v for k, v in critic.items()})
    assert pref.self_dim == plain.self_dim == 35
    for f in plain.actor_p:
        assert pref.actor_p[f] is plain.actor_p[f]
    # a nested mapping (TensorDict keys as tuples / sub-dicts)
    nested = {"module": {}}
    for k, v in actor.items():
        d = nested["module"]
        parts = k.split(".")
        for p in parts[:-1]:
            d = d.setdefault(p, {})
        d[parts[-1]] = v
    assert set(P.DevicePolicy(nested, critic).actor_p) == set(plain.actor_p)


def test_live_modules_and_checkpoints(gp, tmp_path):
    actor, critic = _golden_params(gp, "a3k8d20")

    class Holder(torch.nn.Module):                     # an nn.Module whose named_parameters carry the reference's names under module.
        def __init__(self, params):
            super().__init__()
            self.module = torch.nn.Module()
            for k, v in params.items():
                mod = self.module
                parts = k.split(".")
                for p in parts[:-1]:
                    if not hasattr(mod, p):
                        mod.add_module(p, torch.nn.Module())
                    mod = getattr(mod, p)
                mod.register_parameter(parts[-1], torch.nn.Parameter(v.clone()))

    crit = Holder(critic)
    pol = P.DevicePolicy(FakeTD(actor), crit)
    assert pol.critic_p["head_w"] is crit.module.v_out.weight
    ckpt = {"actor_params": {"module." + k: v for k, v in actor.items()}, "critic": crit.state_dict(), "TP": {}, "value_normalizer": {}}
    path = tmp_path / "checkpoint_final.pt"
    torch.save(ckpt, path)
    for src in (ckpt, str(path)):
        p2 = P.DevicePolicy.from_checkpoint(src)
        assert torch.equal(p2.critic_p["head_w"], crit.module.v_out.weight.detach())
    with pytest.raises(KeyError):
        P.DevicePolicy.from_checkpoint({"TP": {}})


def test_unsupported_configurations_are_refused(gp):
    actor, critic = _golden_params(gp, "a3k5d35")
    for cfg, what in (({"share_actor": False}, "share_actor"), ({"critic_input": "state"}, "critic_input"),
                      ({"actor": {"rnn": {"cls": "gru"}}}, "rnn"), ({"critic": {"rnn": {"cls": "gru"}}}, "rnn"), ({"actor": {"tanh": True}}, "tanh")):
        with pytest.raises(P.PolicyConfigError, match=what):
            P.DevicePolicy(actor, critic, cfg=cfg)
    P.DevicePolicy(actor, critic, cfg={"share_actor": True, "critic_input": "obs", "actor": {"tanh": False}, "critic": {}})
    # the same things seen in the parameters themselves
    stacked = {k: v.expand(3, *v.shape) for k, v in actor.items()}
    with pytest.raises(P.PolicyConfigError, match="share_actor"):
        P.DevicePolicy(stacked, critic)
    with pytest.raises(P.PolicyConfigError, match="rnn"):
        P.DevicePolicy({**actor, "rnn.gru.weight_ih": torch.zeros(3, 128)}, critic)
    central = {k.replace("state_self", "state_drones"): v for k, v in critic.items()}
    with pytest.raises(P.PolicyConfigError):
        P.DevicePolicy(actor, central)
    tanh_actor = {k.replace("act_dist.fc_mean", "act_dist.operator"): v for k, v in actor.items()}
    with pytest.raises(P.PolicyConfigError):
        P.DevicePolicy(tanh_actor, critic)
    wide = dict(actor)
    wide["encoder.linear1.weight"] = torch.zeros(256, 128)
    with pytest.raises(P.PolicyConfigError, match="128"):
        P.DevicePolicy(wide, critic)
    big_head = dict(critic)
    big_head["v_out.weight"] = torch.zeros(2, 128)
    with pytest.raises(P.PolicyConfigError, match="head"):
        P.DevicePolicy(actor, big_head)
    with pytest.raises(P.PolicyConfigError, match="missing"):
        P.DevicePolicy({k: v for k, v in actor.items() if "log_std" not in k}, critic)


def test_observation_shapes_are_checked(gp):
    actor, critic, obs, _, _ = R.golden_case(gp, "a3k5d35")
    pol = P.DevicePolicy({k: torch.from_numpy(v) for k, v in actor.items()}, {k: torch.from_numpy(v) for k, v in critic.items()})
    xs, xo, xc = _obs_t(obs)
    with pytest.raises(ValueError):
        pol.forward(xs[..., :20], xo, xc)
    with pytest.raises(ValueError):
        pol.forward(xs, None, xc)
    with pytest.raises(ValueError):
        pol.forward(xs, xo, xc[..., :4])


def test_new_symbols_are_exported_and_refuse_bad_arguments():
    import __graft_entry__ as g
    lib = ctypes.CDLL(g.build())
    for sym in ("hns_policy_packed_bytes", "hns_policy_pack", "hns_policy_forward"):
        assert sym in abi.EXPORTED_SYMBOLS
        assert hasattr(lib, sym)
    L = abi.load_library()
    per_net = lambda D: 6 * 128 * 128 + 18 * 128 + 12 + (D + 8) * 128
    assert L.hns_policy_packed_bytes(35) == 2 * per_net(35) * 4
    assert L.hns_policy_packed_bytes(0) == 0 and L.hns_policy_packed_bytes(97) == 0
    io = abi.HnsPolicyIo()
    fake = ctypes.c_void_p(1 << 20)
    assert L.hns_policy_forward(fake, 35, 4, 8, 5, ctypes.byref(io), 0, 0, None, None) == abi.HNS_ERR_INVALID_ARG
    assert b"num_agents" in L.hns_last_error()
    assert L.hns_policy_forward(fake, 35, 4, 3, 17, ctypes.byref(io), 0, 0, None, None) == abi.HNS_ERR_INVALID_ARG
    assert b"num_cylinders" in L.hns_last_error()
    assert L.hns_policy_forward(fake, 120, 4, 3, 5, ctypes.byref(io), 0, 0, None, None) == abi.HNS_ERR_INVALID_ARG
    assert b"self_dim" in L.hns_last_error()
    net = abi.HnsPolicyNet()
    assert L.hns_policy_pack(ctypes.byref(net), ctypes.byref(net), 35, 3, fake, None) == abi.HNS_ERR_INVALID_ARG
    assert b"non-NULL" in L.hns_last_error()
