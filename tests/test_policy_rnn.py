"""The recurrent device policy on the CPU (no GPU needed): hns_amd.policy.RecurrentDevicePolicy's restatement against the reference's own
recurrent Actor / Critic (tests/golden/g_policy_rnn.npz), its parameter parsing, and the collector's rnn state.

The collector checks run on test_collector.py's stub env (buffers rewritten in place, episodes of chosen lengths): `is_init` is the previous
step's `done` (all ones after the full reset), and every stored segment, re-run step by step from its STORED start state and the stored
flags, reproduces the stored values bit for bit — a state stored from the wrong slot, or after the step instead of before it, fails that."""
import os

import numpy as np
import pytest
import torch

import policy_reference as R
import policy_rnn_reference as RR
from hns_amd import abi, collector, learner, rnn
from hns_amd import policy as P
from hns_amd.tensordict_shim import _ShimTensorDict as TD
from test_collector import StubEnv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def goldens():
    return tuple(np.load(os.path.join(GOLDEN, n)) for n in ("g_policy.npz", "g_gru.npz", "g_policy_rnn.npz"))


def _t(d):
    return {k: torch.as_tensor(np.asarray(v)) for k, v in d.items()}


def _obs(o):
    return torch.as_tensor(o["state_self"]), torch.as_tensor(o["state_others"]) if "state_others" in o else None, torch.as_tensor(o["cylinders"])


def _net(D=3, A=1, seed=3):
    actor, critic = RR.random_net(D, A, seed)
    return _t(actor), _t(critic)


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", RR.CASES)
def test_the_restatement_reproduces_the_references_recurrent_networks(goldens, tag):
    gp, gg, z = goldens
    actor, critic = RR.golden_params(gp, gg, tag)
    case = RR.golden_case(z, tag)
    pol = P.RecurrentDevicePolicy(_t(actor), _t(critic))
    assert pol.recurrent is True
    T = int(case["shape"][4])
    assert T == (5 if tag == "a3k5d35" else 3) and case["is_init"][0].any()
    ha, hc = torch.as_tensor(case["h0:actor"]), torch.as_tensor(case["h0:critic"])
    for t in range(T):
        out = pol.forward(*_obs(RR.step_obs(case, t)), actor_state=ha, critic_state=hc, is_init=torch.as_tensor(case["is_init"][t]),
                          eps=torch.as_tensor(case["eps"][t]))
        for name in ("loc", "action", "log_prob", "value", "actor_state", "critic_state"):
            err = float((getattr(out, name) - torch.as_tensor(case[name][t])).abs().max())
            assert err <= 1e-5, (tag, t, name, err)
        ha, hc = out.actor_state, out.critic_state           # chained through the restatement's own states
    # the test-side fp64 restatement (the GPU gate's yardstick) agrees with the reference too
    ref = RR.forward(actor, critic, RR.step_obs(case, 0), case["h0:actor"], case["h0:critic"], case["is_init"][0], case["eps"][0])
    for name in RR.OUTPUTS:
        assert float(np.abs(ref[name].numpy() - case[name][0]).max()) <= 1e-5, name


def test_parameters_parse_from_the_reference_names_and_a_checkpoint():
    actor, critic = _net(20, 3)
    pol = P.RecurrentDevicePolicy(actor, critic)
    assert set(pol.actor_rnn) == set(pol.critic_rnn) == set(rnn.FIELDS) and "rnn.cell.weight_ih" not in pol.actor_p
    assert pol.actor_rnn["weight_ih"].data_ptr() == actor["rnn.cell.weight_ih"].data_ptr()          # read in place
    prefixed = P.RecurrentDevicePolicy({"module." + k: v for k, v in actor.items()}, {"module." + k: v for k, v in critic.items()})
    ck = P.RecurrentDevicePolicy.from_checkpoint({"actor_params": actor, "critic": critic})
    o, _ = R.random_obs(2, 3, 5, 20, 1)
    a, b, c = (p.forward(*_obs(o), deterministic=True) for p in (pol, prefixed, ck))
    assert torch.equal(a.loc, b.loc) and torch.equal(a.value, c.value) and torch.equal(a.critic_state, c.critic_state)
    cfg = {"share_actor": True, "critic_input": "obs", "actor": {"rnn": {"cls": "gru"}}, "critic": {"rnn": {"cls": "gru"}}}
    P.RecurrentDevicePolicy(actor, critic, cfg=cfg)
    with pytest.raises(P.PolicyConfigError, match="tanh"):
        P.RecurrentDevicePolicy(actor, critic, cfg={"actor": {"rnn": {"cls": "gru"}, "tanh": True}})


def test_a_missing_or_misshapen_gru_is_refused():
    actor, critic = _net(20, 3)
    plain = {k: v for k, v in critic.items() if not k.startswith("rnn.")}
    with pytest.raises(P.PolicyConfigError, match="no GRU"):
        P.RecurrentDevicePolicy(actor, plain)
    short = {k: v for k, v in actor.items() if k != "rnn.layer_norm.bias"}
    with pytest.raises(P.PolicyConfigError, match="rnn.layer_norm.bias"):
        P.RecurrentDevicePolicy(short, critic)
    wide = dict(actor)
    wide["rnn.cell.weight_hh"] = torch.zeros(3 * 64, 64)
    with pytest.raises(P.PolicyConfigError, match="GRUCell"):
        P.RecurrentDevicePolicy(wide, critic)
    extra = dict(critic)
    extra["rnn.cell.weight_hr"] = torch.zeros(4)
    with pytest.raises(P.PolicyConfigError, match="weight_hr"):
        P.RecurrentDevicePolicy(actor, extra)


def test_device_policy_and_the_learner_still_refuse_the_recurrent_configuration():
    actor, critic = _net(20, 3)
    with pytest.raises(P.PolicyConfigError, match="rnn"):
        P.DevicePolicy(actor, critic)
    with pytest.raises(P.PolicyConfigError, match="rnn"):
        P.DevicePolicy({k: v for k, v in actor.items() if not k.startswith("rnn.")}, critic)
    with pytest.raises(P.PolicyConfigError, match="rnn"):
        P.check_config({"actor": {"rnn": {"cls": "gru"}}})
    pol = P.RecurrentDevicePolicy(actor, critic)
    with pytest.raises(P.PolicyConfigError, match="recurrent"):
        learner.DeviceLearner(None, None, {}, device_policy=pol)
    with pytest.raises(P.PolicyConfigError, match="deterministic"):
        pol.act(None, None, None)


def test_is_init_gives_the_bits_of_a_zero_state_and_none_the_bits_of_zeros():
    actor, critic = _net(20, 3)
    pol = P.RecurrentDevicePolicy(actor, critic)
    o, eps = R.random_obs(5, 3, 5, 20, 2)
    ha, hc = (torch.as_tensor(h) for h in RR.random_states(5, 3, 4))
    flags = torch.tensor([True, False, True, False, False])
    e = torch.as_tensor(eps)
    got = pol.forward(*_obs(o), actor_state=ha, critic_state=hc, is_init=flags, eps=e)
    za, zc = ha.clone(), hc.clone()
    za[flags], zc[flags] = 0, 0
    want = pol.forward(*_obs(o), actor_state=za, critic_state=zc, eps=e)
    plain = pol.forward(*_obs(o), actor_state=ha, critic_state=hc, eps=e)
    for a, b, c in zip(got, want, plain):
        assert torch.equal(a, b)
        assert torch.equal(a[~flags], c[~flags]) and not torch.equal(a[flags], c[flags])
    zeros = pol.forward(*_obs(o), actor_state=torch.zeros_like(ha), critic_state=torch.zeros_like(hc), eps=e)
    for a, b in zip(pol.forward(*_obs(o), eps=e), zeros):
        assert torch.equal(a, b)
    for a, b in zip(pol.forward(*_obs(o), actor_state=ha, critic_state=hc, is_init=torch.ones(5, 1, dtype=torch.bool), eps=e), zeros):
        assert torch.equal(a, b)
    # value_only: the critic's half alone; out_states written in place
    buf = hc.clone()
    vo = pol.forward(*_obs(o), critic_state=buf, is_init=flags, value_only=True, out_states=(None, buf))
    assert vo.action is None and vo.actor_state is None and vo.critic_state is buf
    assert torch.equal(vo.value, got.value) and torch.equal(buf, got.critic_state)
    with pytest.raises(ValueError, match="actor_state"):
        pol.forward(*_obs(o), actor_state=ha[:, :2])
    with pytest.raises(ValueError, match="is_init"):
        pol.forward(*_obs(o), is_init=torch.zeros(4, dtype=torch.bool))


def test_call_reads_and_writes_the_references_keys():
    actor, critic = _net(20, 3)
    pol = P.RecurrentDevicePolicy(actor, critic, seed=4)
    o, _ = R.random_obs(4, 3, 5, 20, 6)
    td = TD({"agents": {"observation": {k: torch.as_tensor(v) for k, v in o.items()}}}, torch.Size([4]))
    first = pol(td)
    assert first is td
    for key, shape in ((("agents", "action"), (4, 3, 4)), ("drone.action_logp", (4, 3, 1)), ("state_value", (4, 3, 1)),
                       ("drone.actor_rnn_state", (4, 3, 128)), ("drone.critic_rnn_state", (4, 3, 128))):
        assert tuple(td[key].shape) == shape, key
    ha, hc = td["drone.actor_rnn_state"].clone(), td["drone.critic_rnn_state"].clone()
    zero = pol.forward(*_obs(o), deterministic=True)
    assert torch.equal(hc, zero.critic_state) and torch.equal(ha, zero.actor_state)                  # absent keys: zeros
    v1 = pol.value(td)                                           # reads the state the call left; writes nothing
    assert torch.equal(td["drone.critic_rnn_state"], hc)
    assert torch.equal(v1, pol.forward(*_obs(o), critic_state=hc, value_only=True).value) and not torch.equal(v1, td["state_value"])
    td["is_init"] = torch.tensor([[True], [False], [False], [True]])
    v2 = pol.value(td)
    assert torch.equal(v2[[0, 3]], td["state_value"][[0, 3]]) and torch.equal(v2[[1, 2]], v1[[1, 2]])
    pol(td, deterministic=True)
    want = pol.forward(*_obs(o), actor_state=ha, critic_state=hc, is_init=td["is_init"], deterministic=True)
    assert torch.equal(td[("agents", "action")], want.loc) and torch.equal(td["drone.actor_rnn_state"], want.actor_state)


def test_the_abi_declares_the_recurrent_entry_points():
    for sym in ("hns_policy_rnn_packed_bytes", "hns_policy_rnn_pack", "hns_policy_forward_rnn"):
        assert sym in abi.EXPORTED_SYMBOLS
    lib = abi.load_library()
    assert lib.hns_policy_rnn_packed_bytes() == 2 * (6 * 128 * 128 + 6 * 128) * 4
    assert lib.hns_abi_version() == 8
    import ctypes as C
    assert C.sizeof(abi.HnsPolicyRnnIo) == 40


# ---------------------------------------------------------------------------------------------------------------------------------------
# the collector's rnn state, on test_collector.py's stub env
def _collector(lengths, T, L, A=1, seed=5):
    actor, critic = _net(3, A, seed)
    env = StubEnv(lengths, A)
    pol = P.RecurrentDevicePolicy(actor, critic, seed=seed)
    return env, pol, collector.DeviceCollector(env, pol, T, rnn_seq_len=L)


def _rerun_segments(pol, st, prev_end=None):
    """Every stored segment step by step from its stored start state and the stored flags: the stored values bit for bit (value_only), and
    the actor's and critic's chain (full deterministic calls) ending on the NEXT segment's stored start state.  Returns the states after the
    last step."""
    d, rk = st.data, st.recurrent_kwargs()
    L, S = rk["rnn_seq_len"], rk["actor_rnn_state"].shape[1]
    end = prev_end
    for s in range(S):
        ha, hc = rk["actor_rnn_state"][:, s].clone(), rk["critic_rnn_state"][:, s].clone()
        if end is not None:
            assert torch.equal(ha, end[0]) and torch.equal(hc, end[1]), f"segment {s} does not start where the previous one ended"
        hv = hc.clone()
        for t in range(s * L, (s + 1) * L):
            obs = (d["obs_self"][:, t], d["obs_others"][:, t] if "obs_others" in d else None, d["obs_cylinders"][:, t])
            flags = rk["is_init"][:, t]
            vo = pol.forward(*obs, critic_state=hv, is_init=flags, value_only=True)
            assert torch.equal(vo.value, d["state_value"][:, t]), f"state_value of step {t} (segment {s})"
            hv = vo.critic_state
            full = pol.forward(*obs, actor_state=ha, critic_state=hc, is_init=flags, deterministic=True)
            ha, hc = full.actor_state, full.critic_state
            assert torch.equal(hc, hv)
        end = (ha, hc)
    return end


@pytest.mark.parametrize("lengths, A", [([4, 4, 4, 4], 1), ([3, 3, 5, 3], 1), ([5, 5, 5], 3)])
def test_collect_stores_is_init_and_the_state_going_into_every_segment(lengths, A):
    N, T, L = len(lengths), 8, 4
    env, pol, col = _collector(lengths, T, L, A)
    end, last_done = None, None
    for call in range(2):
        st = col.collect()
        rk = st.recurrent_kwargs()
        is_init, done = rk["is_init"], st.data["done"]
        assert is_init.shape == (N, T, 1) and is_init.dtype == torch.bool
        assert rk["actor_rnn_state"].shape == rk["critic_rnn_state"].shape == (N, T // L, A, 128)
        if call == 0:
            assert is_init[:, 0].all()
        else:
            assert torch.equal(is_init[:, 0], last_done)
        assert torch.equal(is_init[:, 1:], done[:, :-1])
        assert done.any() and not done.all()
        end = _rerun_segments(pol, st, end)
        last_done = done[:, -1].clone()
        # the bootstrap value's inputs: the state after the last step and the next step's flags
        assert torch.equal(rk["last_critic_rnn_state"], end[1]) and torch.equal(rk["last_is_init"], last_done)
        assert torch.equal(st.last["obs_self"][:, 0, 0, 1], env.progress.where(~last_done[:, 0], torch.tensor(lengths, dtype=torch.float32)))
    assert set(st.learner_kwargs()) == {"obs_self", "obs_others", "obs_cylinders", "action", "log_probs", "state_value", "next_obs_last", "reward", "done"}


def test_a_state_stored_after_the_step_fails_the_segment_rerun():
    """The check has teeth: with the segment store moved behind the policy call (the reference's convention: the state AFTER the step) the
    re-run of the stored segments no longer reproduces the stored values."""
    env, pol, col = _collector([5, 5, 5], 8, 4, 1)
    orig = col._rnn_forward

    def late(t, obs):
        out, pre = orig(t, obs)
        if t % col.rnn_seq_len == 0 and col.storage is not None:
            col.storage.store_segment(t // col.rnn_seq_len, dict(zip(collector.RNN_STATES, col._states)))
        return out, pre
    col._rnn_forward = late
    col.collect()
    st = col.collect()
    with pytest.raises(AssertionError):
        _rerun_segments(pol, st)


def test_restart_begins_again_with_every_flag_set_and_the_option_is_checked():
    env, pol, col = _collector([9, 9], 4, 2)
    col.collect()
    col.restart()
    st = col.collect()
    assert st.data["is_init"][:, 0].all() and not st.data["is_init"][:, 1:].any()
    _rerun_segments(pol, st)
    with pytest.raises(ValueError, match="divide"):
        collector.DeviceCollector(env, pol, 8, rnn_seq_len=3)
    assert collector.DeviceCollector(env, pol, 32).rnn_seq_len == 16
    with pytest.raises(ValueError, match="divide"):
        collector.DeviceCollector(env, pol, 8)                   # the default 16 does not divide 8


def test_a_non_recurrent_policys_storage_has_none_of_the_new_names():
    actor, critic = (_t(p) for p in R.random_net(3, 1, 3))
    env = StubEnv([4, 4, 4])
    col = collector.DeviceCollector(env, P.DevicePolicy(actor, critic), 4)
    st = col.collect()
    assert not st.segments and st.rnn_seq_len is None
    assert not ({"is_init", "actor_rnn_state", "critic_rnn_state"} & (set(st.data) | set(st.last)))
    with pytest.raises(KeyError):
        st.recurrent_kwargs()
    with pytest.raises(ValueError, match="recurrent"):
        collector.DeviceCollector(env, P.DevicePolicy(actor, critic), 4, rnn_seq_len=2)
