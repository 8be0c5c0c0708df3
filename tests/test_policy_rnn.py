"""The recurrent device policy on the CPU (no GPU needed): hns_amd.policy.RecurrentDevicePolicy's restatement against the reference's own
recurrent Actor / Critic (tests/golden/g_policy_rnn.npz), its parameter parsing, and the collector's rnn state.

The collector checks run on test_collector.py's stub env (buffers rewritten in place, episodes of chosen lengths): `is_init` is the previous
step's `done` (all ones after the full reset), and every stored segment, re-run step by step from its STORED start state and the stored
flags, reproduces the stored values bit for bit — a state stored from the wrong slot, or after the step instead of before it, fails that.

Last part: teeth for the device gate of test_hip_policy_rnn.py and test_hip_policy_rnn_edges.py.  The shared cases (policy_rnn_cases.py) cover
what they claim, derived from their seeds; every numerical edge is well posed in the two CPU restatements alone; an fp32 emulation of the
kernels' algorithm (policy_rnn_reference.emulate_step) passes the gate on every chain the device runs, and each of thirteen seeded defects
taken from pol_gru_step's own structure fails it on a named chain (DEFECT_TABLE)."""
import os

import numpy as np
import pytest
import torch

import policy_reference as R
import policy_rnn_cases as PC
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


# ---------------------------------------------------------------------------------------------------------------------------------------
# Does the recurrent device gate have teeth?  policy_rnn_reference.emulate_step is an fp32 restatement of the kernels' algorithm; the cases
# (policy_rnn_cases.py) are the chains the GPU gate runs (test_hip_policy_rnn.py, test_hip_policy_rnn_edges.py).
_FEATURES = {}


def _emulate_chain(tag, defect=None, mode=False):
    """{output: worst gate ratio over the steps} of the emulation along the chain `tag`, its own states feeding its next step (as the device's
    do in chain_gate); mode: eps None."""
    actor, critic, obs, eps, flags, ha, hc = PC.case(tag)
    refs = PC.references(tag, mode)
    worst = dict.fromkeys(RR.OUTPUTS, 0.0)
    for t in range(len(obs)):
        if (tag, t) not in _FEATURES:                            # (the encoder's features do not depend on the defect)
            _FEATURES[tag, t] = R.emulate_features(actor, critic, obs[t])
        out = RR.emulate_step(actor, critic, obs[t], ha, hc, flags[t], None if mode else eps[t], defect, features=_FEATURES[tag, t])
        for name, ratio in RR.gate_ratios(out, *refs[t]).items():
            worst[name] = max(worst[name], ratio)
        ha, hc = out["actor_state"], out["critic_state"]
    return worst


def test_the_sweep_reaches_every_tail_length_agent_count_and_tile_count():
    """Derived from the seeds, not assumed: E A mod 32 takes every residue, every A occurs, the tile counts include 1, 2 and >= 4, and
    residue 0 occurs with one, two and three tiles (FULL_TILES)."""
    shapes = [PC.sweep_shape(s) for s in PC.SWEEP_SEEDS]
    assert [E * A % 32 for E, A, _, _ in shapes] == list(range(32)) == list(PC.SWEEP_SEEDS)
    assert {A for _, A, _, _ in shapes} == set(range(1, 8))
    assert all(1 <= K <= 16 and 1 <= D <= 96 and E >= 1 for E, _, K, D in shapes)
    tiles = {PC.tiles_of(s) for s in shapes}
    assert {1, 2} <= tiles and max(tiles) >= 4 and max(tiles) <= PC.MAX_SWEEP_TILES
    assert {K for _, _, K, _ in shapes} >= {1, 16} and len({A > 1 for _, A, _, _ in shapes}) == 2
    full = [(E * A % 32, PC.tiles_of((E, A, K, D))) for E, A, K, D in shapes + PC.FULL_TILES]
    assert {(0, 1), (0, 2), (0, 3)} <= set(full)
    assert [E * A for E, A, _, _ in PC.FULL_TILES] == [32, 64, 96]
    assert len(set(PC.CASE_TAGS)) == len(PC.CASE_TAGS)
    for tag in PC.SWEEP_TAGS + PC.FULL_TAGS:                     # the chain: no flag, then half of the envs
        flags = PC.case(tag)[4]
        assert len(flags) == 2 and not flags[0].any() and flags[1].sum() == (len(flags[1]) + 1) // 2


@pytest.mark.parametrize("shape", PC.STRADDLE_SHAPES, ids=PC.shape_tag)
def test_the_straddle_shapes_have_tiles_that_start_inside_an_env(shape):
    E, A, _, _ = shape
    rows = E * A
    assert 120 <= rows <= 280 and PC.tiles_of(shape) >= 3
    split = PC.straddling_envs(E, A)
    assert len(split) >= 2 and all(e * A // 32 + 1 == (e * A + A - 1) // 32 for e in split)
    starts = [row0 % A == 0 for row0 in range(0, rows, 32)]
    assert any(starts) and not all(starts)                       # a tile on an env boundary and one that is not
    assert len(split) == sum(not s for s in starts)
    # the split division names another env for some row of every tile that starts inside an env, and only there
    wrong = [row for row in range(rows) if row // 32 * 32 // A + row % 32 // A != row // A]
    assert wrong and {row // 32 for row in wrong} == {t for t, s in enumerate(starts) if not s}
    flags = PC.case("straddle-" + PC.shape_tag(shape))[4][0]
    assert sorted(np.nonzero(flags)[0]) == split
    below = sorted({e - 1 for e in split})
    assert below[0] >= 0 and set(below) != set(split)            # the third flag set of the device test is another one


def test_the_long_chain_and_the_old_shapes_are_what_the_device_files_run():
    assert PC.SHAPES == [(1, 3, 5, 35), (11, 3, 5, 35), (5, 1, 5, 20), (3, 7, 16, 96)] and PC.STEPS == 5
    actor, critic, obs, eps, flags, ha, hc = PC.long_case()
    assert PC.LONG_CHAIN == (11, 3, 5, 35) and len(obs) == len(eps) == len(flags) == 64
    assert [t for t, f in enumerate(flags) if f.any()] == [0, 15, 16, 17, 40, 63] and not any(f.all() for f in flags)
    first = PC.case(PC.LONG_CPU_TAG)
    assert len(first[2]) == 8 and all(np.array_equal(a, b) for a, b in zip(first[4], flags))


@pytest.mark.parametrize("name", PC.EDGES)
def test_every_edge_case_is_well_posed_in_the_reference_alone(name):
    """For each output and step max(e_32, 2^-24 max|ref_64|) <= 1e-4 max|ref_64|: the gate still resolves a relative error of 1e-3, and
    everything is finite.  Measured worst per edge: flat_tokens 5.4e-5 (value), saturated_softmax 4.1e-5 and saturated_gates 4.7e-5 (the
    states), near_flat_norm 5.9e-6 (loc), large_state 2.2e-6, large_obs 6.9e-7, carry 1.3e-7."""
    actor, critic, obs, eps, flags, ha, hc = PC.case(name)
    E, A = PC.EDGE_SHAPES[name][:2]
    assert ha.shape == hc.shape == (E, A, 128) and len(obs) == 3 and 0 < flags[1].sum() < E and not flags[0].any() and not flags[2].any()
    worst = {}
    for r64, r32 in PC.references(name):
        for out in RR.OUTPUTS:
            a, b = r64[out], r32[out]
            assert np.isfinite(a).all() and np.isfinite(b).all()
            top = float(np.abs(a).max())
            bound = max(float(np.abs(b - a).max()), 2.0 ** -24 * top)
            assert bound <= PC.POSED_CAP * top, (name, out, bound / top)
            worst[out] = max(worst.get(out, 0.0), bound / top)
    print(f"  {name}: " + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))
    # the edge is there: what each case is named after, in the fp64 reference
    gru = lambda p, n: np.asarray(p["rnn.cell." + n], np.float64)
    if name == "saturated_gates":
        assert all(np.abs(gru(p, "weight_hh")).max() > 4 for p in (actor, critic))
        s = PC.references(name)[0][0]["actor_state"]
        assert (np.abs(s) > 0.999).mean() > 0.05                 # n = tanh(+-large) behind z ~ 0
    if name == "large_state":
        assert float(np.abs(ha).max()) > 100 and float(np.abs(hc).max()) > 100
    if name == "large_obs":
        assert float(np.abs(obs[0]["state_self"]).max()) > 300


@pytest.mark.parametrize("name", ["carry", "near_flat_norm"])
def test_the_carry_cases_update_gate_is_exactly_one_in_fp32(name):
    """The smallest fp64 z pre-activation over all rows and steps is >= 18: expf(-a) < 2^-24, 1 + expf(-a) rounds to 1 and the fp32 gate is
    exactly 1, so h' = (1 - 1) n + 1 h = h bit for bit (n is finite: a tanh).  near_flat_norm: the sum h0 + f the norm sees is 0.3 within a
    few 1e-2."""
    actor, critic, obs, eps, flags, ha, hc = PC.case(name)
    t64 = lambda p: {k: torch.as_tensor(np.asarray(v)).double() for k, v in p.items()}
    smallest = np.inf
    for p, prefix, key, h0 in ((t64(actor), "encoder.", "actor_state", ha), (t64(critic), "base.", "critic_state", hc)):
        h = torch.as_tensor(h0).double()
        for t in range(len(obs)):
            f = R.encoder(p, prefix, {k: torch.as_tensor(v) for k, v in obs[t].items()}, torch.float64)
            h = h * torch.as_tensor(~flags[t]).double().reshape(-1, 1, 1)
            a_z = (f @ p["rnn.cell.weight_ih"][128:256].T + p["rnn.cell.bias_ih"][128:256]
                   + h @ p["rnn.cell.weight_hh"][128:256].T + p["rnn.cell.bias_hh"][128:256])
            smallest = min(smallest, float(a_z.min()))
            if name == "near_flat_norm" and t == 0:
                flat = (h + f).numpy()
                assert np.abs(flat - 0.3).max() < 0.06 and flat.std(-1).max() < 0.02
            h = torch.as_tensor(PC.references(name)[t][0][key])
            want = h0 if t == 0 else PC.references(name)[t - 1][0][key]
            keep = ~flags[t]
            assert np.abs(h.numpy()[keep] - np.asarray(want, np.float64)[keep]).max() < 1e-7        # fp64: z = 1 - 1e-11
    print(f"  {name}: smallest z pre-activation {smallest:.2f}")
    assert smallest >= 18
    a = torch.tensor(18.0)
    assert float(torch.exp(-a)) < 2.0 ** -24 and float(1.0 / (1.0 + torch.exp(-a))) == 1.0


def test_the_kernels_algorithm_in_fp32_passes_the_gate_on_every_committed_case():
    """No defect: the emulation stays under the bar at every step of every chain the device gate runs — the goldens, the four old shapes, the
    sweep, the full tiles, the straddle shapes, the edges and the first 8 steps of the long chain — sampling and at the mode.  Measured worst
    ratio 2.62 (saturated_gates; saturated_softmax 1.68, the sweep 1.89)."""
    worst = 0.0
    for tag in PC.CASE_TAGS:
        ratios, det = _emulate_chain(tag), _emulate_chain(tag, mode=True)
        for name in RR.OUTPUTS:
            assert ratios[name] <= RR.BAR and det[name] <= RR.BAR, (tag, name, ratios, det)
        worst = max(worst, *ratios.values(), *det.values())
    print(f"  emulate_step, no defect: worst ratio {worst:.2f} of {RR.BAR} over {len(PC.CASE_TAGS)} chains")


def test_a_null_state_all_flags_and_zeros_are_one_thing_to_the_emulation():
    actor, critic, obs, eps, flags, ha, hc = PC.case("random-e11a3k5d35")
    zeros = RR.emulate_step(actor, critic, obs[0], np.zeros_like(ha), np.zeros_like(hc), None, eps[0])
    nan = np.full_like(ha, np.nan)
    for other in (RR.emulate_step(actor, critic, obs[0], None, None, flags[0], eps[0]),
                  RR.emulate_step(actor, critic, obs[0], nan, nan, np.ones(11, bool), eps[0])):        # a flagged row's state is not read
        for name in RR.OUTPUTS + ("action",):
            assert np.array_equal(zeros[name], other[name]), name


# defect -> the committed chain that must fail the gate with it, and the output it fails on.  Measured ratios (bar 8; worst over the chain's
# steps), named case / weakest failing case / cases that still pass, of the 53 chains:
#   flag_env_split_division        straddle-e40a3k5d35 1.4e6 / flat_tokens 3.0e4 / 26: the goldens, the four old shapes, the first 8 steps of the
#                                  long chain (33 rows) and every sweep and full-tile chain in which no tile with a flagged env starts
#                                  inside an env (A 1, 2, 4; one tile; A 5 to 7 over two tiles with the flags elsewhere) — fails on all four
#                                  straddle shapes (> 1e6), all seven edges (A = 3 over five and six tiles), 15 sweep chains and the 96-row full-tile chain
#   flag_by_row                    near_flat_norm 1.6e7 / flat_tokens 3.4e4 / the nine A = 1 chains (row == env)
#   hh_rz_swapped                  large_state 2.8e6 / flat_tokens 3.0e4 / carry, near_flat_norm (z is 1 with either matrix: the state is
#                                  carried and the norm never sees r)
#   bhh_rz_dropped                 a1k5d20 8.2e5 / flat_tokens 4.4e3 / carry, near_flat_norm
#   bhn_outside_r                  a3k5d35 6.3e5 / flat_tokens 5.2e3 / carry, near_flat_norm
#   blend_with_unmasked_h          carry 2.0e7 / flat_tokens 3.4e4 / none
#   mask_after_cell                random-e11a3k5d35 1.5e6 / flat_tokens 2.4e4 / carry, near_flat_norm (h' = h masked before or after)
#   norm_of_old_state              full-e32a2k3d20 2.6e6 / flat_tokens 1.9e4 / carry, near_flat_norm (h' = h)
#   norm_eps_0                     near_flat_norm 3.8e3 / straddle-e40a5k5d35 9.4 / flat_tokens, saturated_softmax, saturated_gates,
#                                  large_state; between 9 and 30 on every ordinary chain (17 to 19 on the old shapes)
#   norm_unbiased_variance         sweep-30-e6a5k7d11 2.2e4 / flat_tokens 206 / none
#   critic_flags_ignored           saturated_gates 4.1e4 / flat_tokens 2.7e4 / none
#   critic_norm_affine_from_actor  long-first8 8.7e5 / flat_tokens 5.2e3 / the goldens (both GRUs carry g_gru.npz's one LayerNorm affine)
#   critic_hh_from_actor_state     random-e1a3k5d35 3.0e6 / flat_tokens 3.1e4 / carry, near_flat_norm
# (flat_tokens is the weakest nearly everywhere because its bound is the largest: e_32 of 3e-5 to 5e-5 of the outputs' size.)
DEFECT_TABLE = {
    "flag_env_split_division": ("straddle-e40a3k5d35", "actor_state"),
    "flag_by_row": ("near_flat_norm", "actor_state"),
    "hh_rz_swapped": ("large_state", "value"),
    "bhh_rz_dropped": ("a1k5d20", "actor_state"),
    "bhn_outside_r": ("a3k5d35", "actor_state"),
    "blend_with_unmasked_h": ("carry", "critic_state"),
    "mask_after_cell": ("random-e11a3k5d35", "actor_state"),
    "norm_of_old_state": ("full-e32a2k3d20", "value"),
    "norm_eps_0": ("near_flat_norm", "loc"),
    "norm_unbiased_variance": (PC.sweep_tag(30), "value"),
    "critic_flags_ignored": ("saturated_gates", "critic_state"),
    "critic_norm_affine_from_actor": (PC.LONG_CPU_TAG, "value"),
    "critic_hh_from_actor_state": ("random-e1a3k5d35", "critic_state"),
}


def test_the_defect_table_names_every_defect():
    assert set(DEFECT_TABLE) == set(RR.DEFECTS) and len(RR.DEFECTS) == 13
    assert all(tag in PC.CASE_TAGS and name in RR.OUTPUTS for tag, name in DEFECT_TABLE.values())
    assert DEFECT_TABLE["flag_env_split_division"][0] in PC.STRADDLE_TAGS and DEFECT_TABLE["norm_eps_0"][0] == "near_flat_norm"


@pytest.mark.parametrize("defect", RR.DEFECTS)
def test_each_seeded_defect_fails_the_gate_on_its_named_case(defect):
    """A subtly wrong kernel does not pass: the same emulation with ONE defect exceeds the bar on the named chain and output; the number of
    chains it fails on, the weakest of them and the ones it still passes are printed."""
    tag, name = DEFECT_TABLE[defect]
    assert max(_emulate_chain(tag).values()) <= RR.BAR
    ratios = _emulate_chain(tag, defect)
    assert ratios[name] > RR.BAR, (defect, tag, ratios)
    worst = {t: max(_emulate_chain(t, defect).values()) for t in PC.CASE_TAGS}
    failing = {t: r for t, r in worst.items() if r > RR.BAR}
    weakest = min(failing, key=failing.get)
    print(f"  {defect}: {tag} {name} {ratios[name]:.3g}; fails on {len(failing)} of {len(worst)} chains, weakest {weakest} {failing[weakest]:.3g}; "
          f"passes {[t for t in worst if t not in failing]}")


def test_the_split_division_passes_the_four_old_shapes_and_fails_every_straddle_shape():
    """The hole the straddle shapes close: reading the flag of row row0 + r at env row0 / A + r / A gives the same answers wherever the tiles
    that hold live rows past r = 0 start on an env boundary — the goldens and all four shapes of test_hip_policy_rnn.py (3, 33, 5, 21 rows)."""
    for tag in list(RR.CASES) + PC.OLD_SHAPE_TAGS:
        clean, split = _emulate_chain(tag), _emulate_chain(tag, "flag_env_split_division")
        assert split == clean and max(split.values()) <= RR.BAR, tag
    for tag in PC.STRADDLE_TAGS:
        assert max(_emulate_chain(tag).values()) <= RR.BAR
        assert min(_emulate_chain(tag, "flag_env_split_division")[n] for n in ("actor_state", "critic_state", "loc", "value")) > 1e3 * RR.BAR, tag
