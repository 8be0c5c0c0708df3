"""Recurrent device evaluation on the CPU (no GPU needed): the refusals of hns_policy_act_rnn, `RecurrentDevicePolicy.act_step`'s restatement
against `forward(deterministic=True)`, and `DeviceEvaluator` with a recurrent policy on test_evaluator.py's stub env.

Refusals: test_evaluator.py's table for hns_policy_act (the shared checks, which this entry runs in the same order) and the entry's own rows,
through ctypes on made-up pointers — HNS_ERR_INVALID_ARG before any launch, the message names the function and the argument; the order of the
checks from calls with two wrong arguments.  act_step: `torch.equal` on the action and the state at every step of a chain that feeds its own
state forward (the golden chains and eval_rnn_cases.py's random ones).  The evaluator: its means and statistics are those of a hand loop that
carries the state through forward(deterministic=True) and NOT those of a loop that drops the state after every step."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import eval_rnn_cases as ERC
import policy_rnn_reference as RR
from hns_amd import abi, collector, evaluator
from hns_amd import policy as P
from hns_amd.tensordict_shim import _ShimTensorDict as TD
from test_evaluator import ACT_REFUSALS, FAKE, StubEnv, StubPolicy, _io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib():
    return abi.load_library()


def _t(d):
    return {k: torch.as_tensor(np.asarray(v)) for k, v in d.items()}


def _obs(o):
    return torch.as_tensor(o["state_self"]), torch.as_tensor(o["state_others"]) if "state_others" in o else None, torch.as_tensor(o["cylinders"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# hns_policy_act_rnn: refusals
def _rio(**kw):
    """An hns_policy_rnn_io that passes every check of hns_policy_act_rnn (the critic's pointers and is_init NULL: the call ignores the
    former and takes NULL for the latter), then `kw` on top."""
    rio = abi.HnsPolicyRnnIo()
    rio.actor_h_in, rio.actor_h_out = FAKE + 32768, FAKE + 49152
    for k, v in kw.items():
        setattr(rio, k, v)
    return rio


GRU = b"null or misaligned packed GRU image / rnn io"
# (what, fragment of the message, overrides of the call, of the io's fields, of the rio's fields)
ACT_RNN_REFUSALS = [r + ({},) for r in ACT_REFUSALS] + [
    ("null rnn image", GRU, dict(rnn_packed=None), {}, {}),
    ("rnn image 8 bytes off 16-byte alignment", GRU, dict(rnn_packed=FAKE + 131072 + 8), {}, {}),
    ("null rio", GRU, dict(rio=None), {}, {}),
    ("rio 4 bytes off 8-byte alignment", GRU, dict(rio_off=4), {}, {}),
    ("actor_h_out missing", b"state output missing or not 16-byte aligned", {}, {}, dict(actor_h_out=None)),
    ("actor_h_out 8 bytes off 16-byte alignment", b"state output missing or not 16-byte aligned", {}, {}, dict(actor_h_out=FAKE + 49152 + 8)),
    ("actor_h_in 8 bytes off 16-byte alignment", b"state input not 16-byte aligned", {}, {}, dict(actor_h_in=FAKE + 32768 + 8)),
    ("actor_h_in 4 bytes off", b"state input not 16-byte aligned", {}, {}, dict(actor_h_in=FAKE + 32768 + 4)),
]


def _refused(lib, call, fields, rfields):
    a = dict(packed=FAKE + 65536, rnn_packed=FAKE + 131072, D=35, E=4, A=3, K=5, io=_io(**fields), rio=_rio(**rfields), rio_off=0)
    a.update(call)
    io = ctypes.byref(a["io"]) if a["io"] is not None else None
    rio = ctypes.byref(a["rio"], a["rio_off"]) if a["rio"] is not None else None
    assert lib.hns_policy_act_rnn(a["packed"], a["rnn_packed"], a["D"], a["E"], a["A"], a["K"], io, rio, None) == abi.HNS_ERR_INVALID_ARG
    err = lib.hns_last_error()
    assert err.startswith(b"hns_policy_act_rnn: "), err
    return err


@pytest.mark.parametrize("row", ACT_RNN_REFUSALS, ids=[r[0].replace(" ", "_") for r in ACT_RNN_REFUSALS])
def test_every_refusal_branch_of_hns_policy_act_rnn(lib, row):
    """One wrong argument at a time on an otherwise valid call.  Every pointer is made up: a row that were NOT refused must never be committed."""
    _, fragment, call, fields, rfields = row
    assert fragment in _refused(lib, call, fields, rfields)


def test_the_refusals_come_in_the_stated_order(lib):
    """Two wrong arguments at a time: the earlier check names itself.  Every call is refused: no pointer here is real."""
    out, h_in = dict(actor_h_out=None), dict(actor_h_in=FAKE + 32768 + 8)
    assert b"num_envs" in _refused(lib, dict(E=0, rnn_packed=None), {}, {})                           # 1 before 2
    assert GRU in _refused(lib, dict(rnn_packed=None), dict(obs_self=None), {})                      # 2 before 3
    assert GRU in _refused(lib, dict(rio=None), dict(action=None), {})
    assert b"observation pointer missing" in _refused(lib, {}, dict(obs_self=None, action=None), {})  # 3 before 4
    assert b"negative stride" in _refused(lib, {}, dict(cyl_stride=(2, -5), action=None), out)
    assert b"action output" in _refused(lib, {}, dict(action=None), out)                              # 4 before 5
    assert b"state output" in _refused(lib, {}, {}, dict(out, **h_in))                                # 5 before 6


def test_the_recurrent_act_entry_is_exported_and_declared(lib):
    assert "hns_policy_act_rnn" in abi.EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "hns.h")).read()
    assert re.search(r"\bint hns_policy_act_rnn\(const void \*packed, const void \*rnn_packed, int32_t self_dim, int64_t num_envs, int32_t num_agents,\s*"
                     r"int32_t num_cylinders,\s*const hns_policy_io \*io, const hns_policy_rnn_io \*rio, void \*stream\);", hdr)
    C = ctypes
    assert lib.hns_policy_act_rnn.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(abi.HnsPolicyIo),
                                               C.POINTER(abi.HnsPolicyRnnIo), C.c_void_p] and lib.hns_policy_act_rnn.restype is C.c_int
    assert lib.hns_abi_version() == 8 and C.sizeof(abi.HnsPolicyRnnIo) == 40                         # purely additive


# ---------------------------------------------------------------------------------------------------------------------------------------
# RecurrentDevicePolicy.act_step on the CPU
def _chain(pol, obs, flags, h0):
    """act_step beside forward(deterministic=True) over a chain, each fed its own state (out of place, then act_step once more with ONE
    persistent action and state tensor written in place): torch.equal at every step."""
    E, A = h0.shape[:2]
    ha = hw = hi = torch.as_tensor(h0)
    hi, out = hi.clone(), torch.full((E, A, 4), 7.0)
    hc = None
    for t in range(len(obs)):
        x, f = _obs(obs[t]), torch.as_tensor(flags[t])
        want = pol.forward(*x, actor_state=hw, critic_state=hc, is_init=f, deterministic=True)
        action, ha = pol.act_step(*x, state=ha, is_init=f)
        assert action.shape == (E, A, 4) and ha.shape == (E, A, 128)
        assert torch.equal(action, want.action) and torch.equal(action, want.loc) and torch.equal(ha, want.actor_state), t
        got = pol.act_step(*x, state=hi, is_init=f, out=out, out_state=hi)
        assert got[0] is out and got[1] is hi and torch.equal(out, want.action) and torch.equal(hi, want.actor_state), t
        hw, hc = want.actor_state, want.critic_state
    assert float(ha.abs().max()) > 0 and float(action.abs().max()) > 0


@pytest.mark.parametrize("tag", RR.CASES)
def test_cpu_act_step_is_the_deterministic_forwards_actor_half_on_the_golden_chains(tag):
    gp, gg, z = (np.load(os.path.join(GOLDEN, n)) for n in ("g_policy.npz", "g_gru.npz", "g_policy_rnn.npz"))
    actor, critic = RR.golden_params(gp, gg, tag)
    case = RR.golden_case(z, tag)
    T = int(case["shape"][4])
    _chain(P.RecurrentDevicePolicy(_t(actor), _t(critic)), [RR.step_obs(case, t) for t in range(T)], list(case["is_init"]), case["h0:actor"])


@pytest.mark.parametrize("shape", ERC.SHAPES, ids=["e%da%dk%dd%d" % s for s in ERC.SHAPES])
def test_cpu_act_step_is_the_deterministic_forwards_actor_half_on_random_chains(shape):
    E, A, K, D = shape
    actor, critic = RR.random_net(D, A, 300 + E + A)
    _chain(P.RecurrentDevicePolicy(_t(actor), _t(critic)), *ERC.random_chain(E, A, K, D, 400 + E))


def test_cpu_act_step_states_flags_outputs_and_what_it_refuses():
    E, A, K, D = 5, 3, 5, 20
    actor, critic = RR.random_net(D, A, 3)
    pol = P.RecurrentDevicePolicy(_t(actor), _t(critic))
    obs, _, h0 = ERC.random_chain(E, A, K, D, 2)
    x, h = _obs(obs[0]), torch.as_tensor(h0)
    zeros = pol.act_step(*x, state=torch.zeros_like(h))
    plain = pol.act_step(*x, state=h)
    assert not torch.equal(plain[0], zeros[0]) and not torch.equal(plain[1], zeros[1])
    for got in (pol.act_step(*x), pol.act_step(*x, state=h, is_init=torch.ones(E, 1, dtype=torch.bool)),
                pol.act_step(*x, state=h, is_init=torch.ones(E, dtype=torch.uint8))):
        assert torch.equal(got[0], zeros[0]) and torch.equal(got[1], zeros[1])          # no state and an all-true is_init: a state of zeros
    flags = torch.tensor([True, False, True, False, False])
    mixed = pol.act_step(*x, state=h, is_init=flags)
    for m, zr, pl in zip(mixed, zeros, plain):
        assert torch.equal(m[flags], zr[flags]) and torch.equal(m[~flags], pl[~flags])
    # out and out_state are written in place and returned; out_state may be the state
    out, new = torch.full((E, A, 4), 7.0), torch.full((E, A, 128), 7.0)
    kept = h.clone()
    got = pol.act_step(*x, state=h, out=out, out_state=new)
    assert got[0] is out and got[1] is new and torch.equal(out, plain[0]) and torch.equal(new, plain[1]) and torch.equal(h, kept)
    got = pol.act_step(*x, state=kept, out_state=kept)
    assert got[1] is kept and torch.equal(kept, plain[1]) and torch.equal(got[0], plain[0])
    for kw, match in ((dict(state=h[:, :2]), "^state must be"), (dict(state=h.double()), "^state must be"),
                      (dict(out_state=h[:, :, :64]), "out_state must be"), (dict(out_state=h.transpose(0, 1).contiguous().transpose(0, 1)), "out_state must be"),
                      (dict(out=out[:, :, :3]), "out must be"), (dict(out=out.double()), "out must be"), (dict(out=out[:-1]), "out must be"),
                      (dict(is_init=torch.zeros(E - 1, dtype=torch.bool)), "is_init must hold"), (dict(is_init=[True] * E), "is_init must hold")):
        with pytest.raises(ValueError, match=match):
            pol.act_step(*x, **kw)
    with pytest.raises(ValueError, match="cylinders must be"):                          # the same checks as forward
        pol.act_step(x[0], x[1], torch.zeros(E, A, 17, 5))
    with pytest.raises(P.PolicyConfigError, match="no actor-only pass; use forward"):   # act keeps refusing: it has no state argument
        pol.act(*x)


# ---------------------------------------------------------------------------------------------------------------------------------------
# DeviceEvaluator with a recurrent policy, on test_evaluator.py's stub env (one agent, rows of 3, two cylinders)
L_EP, N_ENVS = 5, 7


def _stub_policy(seed=21):
    actor, critic = RR.random_net(3, 1, seed)
    actor["act_dist.fc_mean.weight"] = actor["act_dist.fc_mean.weight"] * 30.0          # actions of order 0.3
    return P.RecurrentDevicePolicy(_t(actor), _t(critic), seed=seed)


def _step_input(env):
    return lambda action: TD({"agents": {"action": action}}, env.batch_size)


def test_evaluate_carries_the_actor_state_and_puts_everything_back():
    pol = _stub_policy()
    env, hand, amnesic = (StubEnv([L_EP] * N_ENVS, L_EP) for _ in range(3))
    calls = []
    act_step = pol.act_step
    pol.act_step = lambda *a, **kw: (calls.append(kw), act_step(*a, **kw))[1]
    ev = evaluator.DeviceEvaluator(env, pol)
    torch.manual_seed(1234)
    torch.rand(5)
    before, gen = torch.get_rng_state().clone(), pol._generator.get_state().clone()
    info = ev.evaluate(seed=3)
    assert torch.equal(torch.get_rng_state(), before) and torch.equal(pol._generator.get_state(), gen)
    assert (env.training, env.seed, env.reset_epoch) == (False, 11, 3)                  # everything _save / _restore covers
    assert (ev.steps, ev.done_reads, env.steps, env.full_resets, env.masked_resets, len(calls)) == (L_EP, 1, L_EP, 1, 0, L_EP)
    # step 0 from no state (the full reset), then ONE state and ONE action tensor in place, never an is_init tensor
    assert calls[0]["state"] is None and calls[0]["out"] is None and calls[0]["out_state"] is None
    state, action = calls[1]["state"], calls[1]["out"]
    assert tuple(state.shape) == (N_ENVS, 1, 128) and tuple(action.shape) == (N_ENVS, 1, 4)
    assert all(c["state"] is state and c["out_state"] is state and c["out"] is action for c in calls[1:])
    assert all("is_init" not in c for c in calls)
    # the hand loops
    cur = ERC.hand_loop(hand, pol, 3, _step_input(hand), stateful=True)
    ERC.hand_loop(amnesic, pol, 3, _step_input(amnesic), stateful=False)
    assert set(info) == {"eval/stats.score", "eval/stats.gap"} and set(ev.stats) == {"score", "gap"}
    want, _, _ = evaluator.stat_means([hand.stats["score"], hand.stats["gap"]], cur["done"])
    assert info["eval/stats.score"] == float(want[0]) and info["eval/stats.gap"] == float(want[1]) == L_EP / 2
    assert torch.equal(ev.stats["score"], hand.stats["score"].reshape(-1))
    # the teeth: a loop that zeroes the state on every step gives other statistics and another mean
    assert not torch.equal(hand.stats["score"], amnesic.stats["score"])
    assert not torch.equal(ev.stats["score"], amnesic.stats["score"].reshape(-1))
    assert info["eval/stats.score"] != float(evaluator.stat_means([amnesic.stats["score"]], None)[0][0])
    again = ev.evaluate(seed=3)
    assert again == info and (ev.steps, ev.done_reads) == (2 * L_EP, 2) and calls[L_EP]["state"] is None       # every run starts from zeros


def test_a_recurrent_collector_restarts_from_a_full_reset_with_every_flag_set():
    T = 2
    pol = _stub_policy()
    env = StubEnv([L_EP] * N_ENVS, L_EP)
    col = collector.DeviceCollector(env, pol, T, rnn_seq_len=T)
    col.collect()
    st = col.collect()
    assert env.full_resets == 1 and not st.data["is_init"].any()                        # mid-episode: no flag anywhere in the rollout
    states = tuple(s.clone() for s in col._states)
    evaluator.DeviceEvaluator(env, pol, collector=col).evaluate(seed=2)
    assert env.full_resets == 2 and all(torch.equal(a, b) for a, b in zip(col._states, states))       # the collector's own states: untouched
    st = col.collect()
    assert env.full_resets == 3 and col._since_full_reset == T
    assert st.data["is_init"][:, 0].all() and not st.data["is_init"][:, 1:].any()
    assert st.data["obs_self"][:, 0, 0, 0, 1].tolist() == [0.0] * N_ENVS
    # ... so slot 0 holds what a zero state gives, whatever the states held
    x = (st.data["obs_self"][:, 0], None, st.data["obs_cylinders"][:, 0])
    assert torch.equal(st.data["state_value"][:, 0], pol.forward(*x, value_only=True).value)


def test_a_non_recurrent_policy_still_goes_through_act():
    env, pol = StubEnv([L_EP] * N_ENVS, L_EP), StubPolicy()
    assert not hasattr(pol, "act_step") and not getattr(pol, "recurrent", False)
    ev = evaluator.DeviceEvaluator(env, pol)
    info = ev.evaluate(seed=3)
    assert pol.acts == L_EP and pol.same_out and (ev.steps, ev.done_reads) == (L_EP, 1)
    assert info["eval/stats.gap"] == L_EP / 2
