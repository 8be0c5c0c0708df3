"""Recurrent per-agent actors on an MI355X (share_actor: False with actor.rnn / critic.rnn): hns_policy_rnn_pack_agents,
hns_policy_forward_rnn_agents and hns_policy_act_rnn_agents through hns_amd.policy.PerAgentRecurrentDevicePolicy and through the C ABI, the
collector and the evaluator with that policy.

The property everything stands on: for every agent a, every output of row (e, a) — action, loc, log_prob, value, both states — is BIT FOR BIT
what hns_policy_forward_rnn writes for that row on the images of (agent a's slices, critic), for the same inputs, eps or seed and counter, and
flags.  A row's result does not depend on the rows it shares a tile with, so no tolerance is involved: A shared-entry calls on the slices are
the reference.  The shapes put 1, 31, 32 and 33 envs in an agent's tiles (one live row; one short of a tile; a full tile; a second tile with one
live row), 97 envs of one-value observations over four tiles, every limit at its maximum, and one agent without state_others.

Beside it the project's fp64 gate (per output, e_hip <= 8 max(e_32, 2^-24 max|ref_64|) against tests/policy_rnn_reference.py's restatement run
per slice) on the two cases of g_policy_rnn_per_agent.npz and one random 33-env chain, the device's own states feeding its next call."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_rnn_cases as ERC
import learner_cases as LC
import per_agent_rnn_cases as PR
import policy_reference as R
import policy_rnn_reference as RR
from hns_amd import abi, collector, config, evaluator
from hns_amd import policy as P
from hns_amd.tensordict_shim import TensorDict

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(1, 3, 5, 35), (31, 3, 5, 35), (32, 3, 5, 35), (33, 3, 5, 35), (97, 2, 1, 1), (5, 7, 16, 96), (40, 1, 5, 20)]      # (E, A, K, D)
S33 = (33, 3, 5, 35)
FIELDS = P.RecurrentPolicyOutput._fields
VO, DET = abi.HNS_POLICY_VALUE_ONLY, abi.HNS_POLICY_DETERMINISTIC
BAR = RR.BAR
RATIOS = {}
SEED = 11


def _tag(shape):
    return "e%da%dk%dd%d" % tuple(shape)


def _cuda(x):
    return torch.as_tensor(np.asarray(x)).cuda() if x is not None else None


def _obs_dev(obs):
    return _cuda(obs["state_self"]), _cuda(obs.get("state_others")), _cuda(obs["cylinders"])


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _policies(actors, critic):
    """(the per-agent policy, the A shared recurrent policies on the agents' slices — views of the same device tensors) at one seed."""
    da, dc = {k: _cuda(v) for k, v in actors.items()}, {k: _cuda(v) for k, v in critic.items()}
    A = next(iter(da.values())).shape[0]
    pol = P.PerAgentRecurrentDevicePolicy(da, dc, seed=SEED)
    slices = [P.RecurrentDevicePolicy({k: v[a] for k, v in da.items()}, dc, seed=SEED) for a in range(A)]
    return pol, slices, da, dc


@functools.lru_cache(maxsize=None)
def _setup(shape):
    """(policy, slice policies, observation, eps, start states, mixed flags) of a shape, built once per process (read-only)."""
    E, A, K, D = shape
    actors, critic = PR.random_net(D, A, 900 + E + A)
    pol, slices, _, _ = _policies(actors, critic)
    obs, eps = R.random_obs(E, A, K, D, 910 + E)
    ha, hc = (_cuda(h) for h in RR.random_states(E, A, 920 + E))
    return pol, slices, _obs_dev(obs), _cuda(eps), ha, hc, _cuda(PR.random_flags(E, 930 + E))


def _slice_rows(slices, x, **kw):
    """Row (e, a) from slice a's shared-entry call on the whole batch: the reference of the property (value and the critic's state from
    agent 0's call; every call's are checked to be the same bits, the critic being shared)."""
    outs = [s.forward(*x, **kw) for s in slices]
    rows = {}
    for f in FIELDS:
        if getattr(outs[0], f) is None:
            rows[f] = None
        elif f in ("value", "critic_state"):
            assert all(_bits(getattr(o, f), getattr(outs[0], f)) for o in outs), f
            rows[f] = getattr(outs[0], f)
        else:
            rows[f] = torch.stack([getattr(o, f)[:, a] for a, o in enumerate(outs)], dim=1)
    return rows


def _same(got, want, what):
    for f in FIELDS:
        g, w = getattr(got, f), want[f]
        assert (g is None) == (w is None), (what, f)
        if g is not None:
            assert bool(torch.isfinite(g).all()), (what, f)
            assert _bits(g, w), (what, f, int((g != w).sum()))


def _set_counters(pol, slices, c):
    for p in (pol, *slices):
        p.counter.fill_(c)


# ---- 1. the property -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_tag)
def test_row_e_a_is_the_shared_entrys_row_on_agent_as_images_bit_for_bit(shape):
    """Sampling with eps and deterministic at every shape, states given and flags mixed; act_step is the deterministic forward's actor half;
    at A = 1 the whole batch through hns_policy_forward_rnn is the same bits."""
    pol, slices, x, eps, ha, hc, flags = _setup(shape)
    kw = dict(actor_state=ha, critic_state=hc, is_init=flags)
    sampled = pol.forward(*x, eps=eps, **kw)
    _same(sampled, _slice_rows(slices, x, eps=eps, **kw), "eps")
    det = pol.forward(*x, deterministic=True, **kw)
    _same(det, _slice_rows(slices, x, deterministic=True, **kw), "deterministic")
    assert _bits(det.action, det.loc) and _bits(det.loc, sampled.loc) and not _bits(sampled.action, sampled.loc)
    c0 = pol.counter.clone()
    action, state = pol.act_step(*x, state=ha, is_init=flags)
    assert _bits(action, det.action) and _bits(state, det.actor_state) and torch.equal(pol.counter, c0)
    if shape[1] == 1:
        whole = slices[0].forward(*x, eps=eps, **kw)
        assert all(_bits(getattr(sampled, f), getattr(whole, f)) for f in FIELDS)
    else:                                                        # the agents' images are not interchangeable
        assert not _bits(det.loc[:, 0], slices[1].forward(*x, deterministic=True, **kw).loc[:, 0])


def test_every_mode_at_33_envs():
    """Sampling by Philox (the same seed and counter), value-only, and the noise scheme's row numbering e A + a."""
    pol, slices, x, eps, ha, hc, flags = _setup(S33)
    kw = dict(actor_state=ha, critic_state=hc, is_init=flags)
    c0 = int(pol.counter)
    _set_counters(pol, slices, c0 + 5)
    got = pol.forward(*x, **kw)
    assert int(pol.counter) == c0 + 6                            # one bump per sampling call without eps
    want = _slice_rows(slices, x, **kw)                          # (each slice's counter: c0 + 5 as well)
    _same(got, want, "philox")
    z = ((got.action - got.loc) / pol.scale.unsqueeze(0)).cpu().numpy().reshape(-1, 4)
    assert np.abs(z - R.philox_normal(pol.seed, c0 + 5, z.shape[0], np.float32)).max() < 1e-3        # counter (call, e A + a)
    again = pol.forward(*x, **kw)
    assert int(pol.counter) == c0 + 7 and not _bits(again.action, got.action) and _bits(again.loc, got.loc)
    c = pol.counter.clone()
    pol.forward(*x, eps=eps, **kw), pol.forward(*x, deterministic=True, **kw), pol.forward(*x, critic_state=hc, value_only=True)
    pol.act_step(*x, state=ha)
    assert torch.equal(pol.counter, c)                           # ... and it moves in no other call
    vo = pol.forward(*x, critic_state=hc, is_init=flags, value_only=True)
    assert vo.action is None and vo.actor_state is None
    assert _bits(vo.value, got.value) and _bits(vo.critic_state, got.critic_state)
    _set_counters(pol, slices, c0)


STATE_FORMS = [(s, f) for s in ("null", "given", "in place") for f in ("null", "mixed", "ones")]


@pytest.mark.parametrize("states, flagged", STATE_FORMS, ids=["%s states, %s flags" % sf for sf in STATE_FORMS])
def test_states_and_flags_at_33_envs(states, flagged):
    """States NULL, given and in place (h_out == h_in) with is_init NULL, mixed and all ones: the slices' bits; NaN in the stale state of a
    flagged env reaches no output; a flagged env's rows are those of a zero state."""
    pol, slices, x, eps, ha, hc, mixed = _setup(S33)
    E, A = ha.shape[:2]
    flags = {"null": None, "mixed": mixed, "ones": torch.ones(E, dtype=torch.bool, device="cuda")}[flagged]
    if states == "null":
        got = pol.forward(*x, is_init=flags, eps=eps)
        _same(got, _slice_rows(slices, x, is_init=flags, eps=eps), "null states")
        zero = torch.zeros_like(ha)
        assert _bits(got.loc, pol.forward(*x, actor_state=zero, critic_state=zero, eps=eps).loc)
        return
    na, nc = ha.clone(), hc.clone()
    if flags is not None:
        na[flags], nc[flags] = float("nan"), float("nan")        # the stale state of a flagged env is not read
    want = _slice_rows(slices, x, actor_state=ha, critic_state=hc, is_init=flags, eps=eps)
    if states == "given":
        got = pol.forward(*x, actor_state=na, critic_state=nc, is_init=flags, eps=eps)
        action, state = pol.act_step(*x, state=na, is_init=flags)
    else:
        ia, ic, sa = na.clone(), nc.clone(), na.clone()
        got = pol.forward(*x, actor_state=ia, critic_state=ic, is_init=flags, eps=eps, out_states=(ia, ic))
        assert got.actor_state is ia and got.critic_state is ic
        action, state = pol.act_step(*x, state=sa, is_init=flags, out_state=sa)
        assert state is sa
    _same(got, want, f"{states}, {flagged}")
    assert _bits(action, want["loc"]) and _bits(state, want["actor_state"])
    if flags is not None:
        za, zc = ha.clone(), hc.clone()
        za[flags], zc[flags] = 0, 0
        zeroed = pol.forward(*x, actor_state=za, critic_state=zc, eps=eps)
        assert all(_bits(getattr(got, f), getattr(zeroed, f)) for f in FIELDS)
        plain = pol.forward(*x, actor_state=ha, critic_state=hc, eps=eps)
        assert _bits(got.loc[~flags], plain.loc[~flags]) and bool((got.loc[flags] != plain.loc[flags]).flatten(1).any(1).all())


# ---- 2. through the C ABI: what a call writes and what it leaves alone ----------------------------------------------------------------
SENTINEL = 777.0
WIDTH = {"action": 4, "log_prob": 1, "loc": 4, "value": 1, "actor_h_out": 128, "critic_h_out": 128}


def _c_call(pol, x, ha, hc, flags, mode, eps=None):
    """One call of hns_policy_forward_rnn_agents (mode "sample", "det", "value_only") or hns_policy_act_rnn_agents ("act") with every output
    pointer set to a sentinel-filled buffer.  -> {name: [E, A, width] tensor}."""
    pol.refresh()
    xs, xo, xc, io = pol._io(x[0].squeeze(2), x[1], x[2])
    E, A, K = xs.shape[0], xs.shape[1], xc.shape[2]
    bufs = {n: torch.full((E, A, w), SENTINEL, device="cuda") for n, w in WIDTH.items()}
    io.action, io.log_prob, io.loc, io.value = (bufs[n].data_ptr() for n in ("action", "log_prob", "loc", "value"))
    io.eps = eps.data_ptr() if eps is not None else None
    rio = abi.HnsPolicyRnnIo()
    rio.actor_h_in, rio.critic_h_in = ha.data_ptr() if ha is not None else None, hc.data_ptr() if hc is not None else None
    rio.actor_h_out, rio.critic_h_out = bufs["actor_h_out"].data_ptr(), bufs["critic_h_out"].data_ptr()
    rio.is_init = flags.view(torch.uint8).data_ptr() if flags is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if mode == "act":
        rc = pol._lib.hns_policy_act_rnn_agents(pol.packed.data_ptr(), pol.rnn_packed.data_ptr(), pol.self_dim, E, A, K, C.byref(io), C.byref(rio), st)
    else:
        bits = {"sample": 0, "det": DET, "value_only": VO}[mode]
        rc = pol._lib.hns_policy_forward_rnn_agents(pol.packed.data_ptr(), pol.rnn_packed.data_ptr(), pol.self_dim, E, A, K, C.byref(io), C.byref(rio),
                                                    bits, pol.seed, pol.counter.data_ptr(), st)
    assert rc == abi.HNS_OK, pol._lib.hns_last_error()
    torch.cuda.synchronize()
    return bufs


def _untouched(t):
    return bool((t == SENTINEL).all())


def test_value_only_and_act_write_only_what_is_theirs():
    """Value-only: action, log_prob, loc and actor_h_out keep the sentinel and a NaN-filled actor_h_in is not read.  act: action and
    actor_h_out are the deterministic forward's bits; log_prob, value, loc, the critic's state and the counter are untouched, and a
    NaN-filled critic_h_in is not read."""
    pol, _, x, eps, ha, hc, flags = _setup(S33)
    nan = torch.full_like(ha, float("nan"))
    c0 = pol.counter.clone()
    full = _c_call(pol, x, ha, hc, flags, "sample", eps)
    assert not any(_untouched(t) for t in full.values())
    vo = _c_call(pol, x, nan, hc, flags, "value_only", eps)
    for n in ("action", "log_prob", "loc", "actor_h_out"):
        assert _untouched(vo[n]), n
    assert _bits(vo["value"], full["value"]) and _bits(vo["critic_h_out"], full["critic_h_out"])
    det = _c_call(pol, x, ha, hc, flags, "det")
    act = _c_call(pol, x, ha, nan, flags, "act")
    assert _bits(act["action"], det["action"]) and _bits(act["actor_h_out"], det["actor_h_out"])
    for n in ("log_prob", "loc", "value", "critic_h_out"):
        assert _untouched(act[n]), n
    assert torch.equal(pol.counter, c0)
    # the class writes the same bits as the C call
    out = pol.forward(*x, actor_state=ha, critic_state=hc, is_init=flags, eps=eps)
    assert _bits(out.action, full["action"]) and _bits(out.log_prob, full["log_prob"]) and _bits(out.actor_state, full["actor_h_out"])


# ---- 3. the packed GRU images ----------------------------------------------------------------------------------------------------------
def test_each_gru_image_is_its_half_of_the_shared_pack_and_follows_an_in_place_update():
    E, A, K, D = 5, 3, 5, 35
    actors, critic = PR.random_net(D, A, 940)
    pol, slices, da, dc = _policies(actors, critic)
    obs, eps = R.random_obs(E, A, K, D, 941)
    x, e = _obs_dev(obs), _cuda(eps)
    ha, hc = (_cuda(h) for h in RR.random_states(E, A, 942))

    def images():
        pol.refresh()
        torch.cuda.synchronize()
        return pol.rnn_packed.view(A + 1, -1), pol.packed.view(A + 1, -1)

    def check():
        rnn, enc = images()
        assert pol.rnn_packed.numel() == pol._lib.hns_policy_rnn_packed_agents_bytes(A) == (A + 1) * pol._lib.hns_policy_rnn_packed_bytes() // 2
        for a, s in enumerate(slices):
            s.refresh()
            torch.cuda.synchronize()
            half, ehalf = s.rnn_packed.view(2, -1), s.packed.view(2, -1)
            assert torch.equal(rnn[a], half[0]), f"actor GRU image {a}"
            assert torch.equal(rnn[A], half[1]), f"critic GRU image (against slice {a}'s)"
            assert torch.equal(enc[a], ehalf[0]) and torch.equal(enc[A], ehalf[1]), f"encoder images (slice {a})"
        assert not torch.equal(rnn[0], rnn[1]) and not torch.equal(rnn[0], rnn[A])
    check()
    before = pol.forward(*x, actor_state=ha, critic_state=hc, eps=e)
    da["rnn.cell.weight_hh"][1].mul_(0.5)                        # ONE agent's GRU weight, in place: the version counter moves
    mid = pol.forward(*x, actor_state=ha, critic_state=hc, eps=e)
    assert _bits(mid.loc[:, 0], before.loc[:, 0]) and _bits(mid.loc[:, 2], before.loc[:, 2]) and not _bits(mid.loc[:, 1], before.loc[:, 1])
    assert _bits(mid.value, before.value)
    dc["rnn.cell.bias_ih"].add_(0.25)                            # ... then the shared critic's GRU
    da["encoder.linear1.weight"][2].mul_(0.5)                    # ... and an encoder weight of agent 2
    after = pol.forward(*x, actor_state=ha, critic_state=hc, eps=e)
    assert _bits(after.loc[:, :2], mid.loc[:, :2]) and not _bits(after.loc[:, 2], mid.loc[:, 2]) and not _bits(after.value, mid.value)
    check()                                                      # the slices' views see the same tensors: their images moved alike
    _same(after, _slice_rows(slices, x, actor_state=ha, critic_state=hc, eps=e), "after the updates")


# ---- 4. the fp64 gate -------------------------------------------------------------------------------------------------------------------
def _golden_chain(tag):
    gp, gg, z = (np.load(os.path.join(GOLDEN, n)) for n in ("g_policy.npz", "g_gru.npz", "g_policy_rnn_per_agent.npz"))
    actors, critic, case = PR.golden_case(z, gp, gg, tag)
    T = int(case["shape"][4])
    return actors, critic, [RR.step_obs(case, t) for t in range(T)], list(case["eps"]), list(case["is_init"]), case["h0:actor"], case["h0:critic"]


def _random_chain():
    E, A, K, D = S33
    actors, critic = PR.random_net(D, A, 950)
    obs, eps = zip(*(R.random_obs(E, A, K, D, 951 + t) for t in range(3)))
    flags = [PR.random_flags(E, 955), np.zeros(E, bool), PR.random_flags(E, 956)]
    return (actors, critic, list(obs), list(eps), flags, *RR.random_states(E, A, 957))


@pytest.mark.parametrize("tag", PR.CASES + ("random-" + _tag(S33),))
def test_the_fp64_gate_along_a_self_fed_chain(tag):
    """e_hip <= 8 max(e_32, 2^-24 max|ref_64|) for loc, log_prob, value and both states at every step, against the fp64 restatement run per
    slice."""
    actors, critic, obs, eps, flags, ha, hc = _golden_chain(tag) if tag in PR.CASES else _random_chain()
    refs = PR.chain_references(actors, critic, obs, eps, flags, ha, hc)
    pol = _policies(actors, critic)[0]
    da, dc = _cuda(ha), _cuda(hc)
    for t in range(len(obs)):
        out = pol.forward(*_obs_dev(obs[t]), actor_state=da, critic_state=dc, is_init=_cuda(flags[t]), eps=_cuda(eps[t]))
        got = {n: getattr(out, n).cpu().double().numpy() for n in RR.OUTPUTS}
        ratios = RR.gate_ratios(got, *refs[t])
        print(f"  {tag} step {t}: " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
        for name, ratio in ratios.items():
            assert ratio <= BAR, f"{tag} step {t} {name}: ratio {ratio:.2f} > {BAR}"
        RATIOS[tag] = max(RATIOS.get(tag, 0.0), *ratios.values())
        da, dc = out.actor_state, out.critic_state
    print(f"  {tag}: worst ratio {RATIOS[tag]:.2f}")


# ---- 5. no host synchronisation ---------------------------------------------------------------------------------------------------------
def test_forward_and_act_step_make_no_host_synchronisation():
    pol, _, x, eps, ha, hc, flags = _setup(S33)
    pol.refresh()
    oa, oc, action = torch.empty_like(ha), torch.empty_like(hc), torch.empty(ha.shape[0], ha.shape[1], 4, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pol.forward(*x, actor_state=ha, critic_state=hc, is_init=flags, out_states=(oa, oc))
        pol.forward(*x, actor_state=ha, critic_state=hc, is_init=flags, eps=eps)
        pol.forward(*x, critic_state=hc, value_only=True)
        pol.act_step(*x, state=ha, is_init=flags, out=action, out_state=oa)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(action).all()) and bool(torch.isfinite(oa).all())


# ---- 6. the C entries' refusals ---------------------------------------------------------------------------------------------------------
def _refused(pol, x, entry="forward", over=None, rover=None, flags=0, packed=True, rnn_packed=True, io=True, rio=True, counter=True, shape=None):
    """One call with sentinel-filled buffers; `over` / `rover` replace io / rio fields (an int: an offset added to the pointer).
    -> (rc, message, nothing was written and the counter did not move)."""
    pol.refresh()
    xs, xo, xc, pio = pol._io(x[0].squeeze(2), x[1], x[2])
    E, A, K = xs.shape[0], xs.shape[1], xc.shape[2]
    sent = lambda *s: torch.full(s, SENTINEL, device="cuda")     # noqa: E731
    bufs = {"action": sent(E, A, 4), "log_prob": sent(E, A), "loc": sent(E, A, 4), "value": sent(E, A), "actor_h_out": sent(E, A, 128 + 4),
            "critic_h_out": sent(E, A, 128 + 4), "actor_h_in": sent(E, A, 128 + 4), "critic_h_in": sent(E, A, 128 + 4)}
    for n in ("action", "log_prob", "loc", "value"):
        setattr(pio, n, bufs[n].data_ptr())
    prio = abi.HnsPolicyRnnIo()
    for n in ("actor_h_out", "critic_h_out", "actor_h_in", "critic_h_in"):
        setattr(prio, n, bufs[n].data_ptr())
    for k, v in (over or {}).items():
        if isinstance(v, tuple):
            getattr(pio, k)[v[0]] = v[1]
        else:
            setattr(pio, k, (getattr(pio, k) or 0) + v if isinstance(v, int) and v else v)
    for k, v in (rover or {}).items():
        setattr(prio, k, getattr(prio, k) + v if isinstance(v, int) and v else v)
    D, E_, A_, K_ = shape or (pol.self_dim, E, A, K)
    off = lambda v: v if isinstance(v, int) and not isinstance(v, bool) else 0          # noqa: E731
    pk = pol.packed.data_ptr() + off(packed) if packed else None
    rk = pol.rnn_packed.data_ptr() + off(rnn_packed) if rnn_packed else None
    pio_ref = C.byref(pio) if io else None
    prio_ref = (C.byref(prio, off(rio))) if rio else None
    c0 = int(pol.counter)
    if entry == "forward":
        rc = pol._lib.hns_policy_forward_rnn_agents(pk, rk, D, E_, A_, K_, pio_ref, prio_ref, flags, pol.seed, pol.counter.data_ptr() if counter else None, None)
    else:
        rc = pol._lib.hns_policy_act_rnn_agents(pk, rk, D, E_, A_, K_, pio_ref, prio_ref, None)
    torch.cuda.synchronize()
    return rc, pol._lib.hns_last_error().decode(), all(_untouched(t) for t in bufs.values()) and int(pol.counter) == c0


REFUSALS = [
    # hns_policy_forward_rnn's, in its order
    ("null packed image", dict(packed=False), "packed image"), ("misaligned packed image", dict(packed=4), "packed image"),
    ("null io", dict(io=False), "packed image / io"), ("self_dim 0", dict(shape=(0, 33, 3, 5)), "self_dim"),
    ("self_dim 97", dict(shape=(97, 33, 3, 5)), "self_dim"), ("8 agents", dict(shape=(35, 33, 8, 5)), "num_agents"),
    ("0 agents", dict(shape=(35, 33, 0, 5)), "num_agents"), ("17 cylinders", dict(shape=(35, 33, 3, 17)), "num_cylinders"),
    ("0 envs", dict(shape=(35, 0, 3, 5)), "num_envs"),
    ("null rnn image", dict(rnn_packed=False), "GRU image"), ("misaligned rnn image", dict(rnn_packed=4), "GRU image"),
    ("null rio", dict(rio=False), "rnn io"), ("misaligned rio", dict(rio=4), "rnn io"),
    ("unknown flag", dict(flags=4), "flag"),
    ("missing obs_self", dict(over={"obs_self": None}), "observation"), ("missing obs_others", dict(over={"obs_others": None}), "observation"),
    ("misaligned cylinders", dict(over={"obs_cylinders": 2}), "misaligned observation"),
    ("negative stride", dict(over={"cyl_stride": (1, -1)}), "negative stride"),
    ("missing value", dict(over={"value": None}), "value"), ("missing action", dict(over={"action": None}), "action"),
    ("misaligned log_prob", dict(over={"log_prob": 2}), "action / log_prob"), ("sampling without a counter", dict(counter=False), "counter"),
    ("missing critic_h_out", dict(rover={"critic_h_out": None}), "state output"), ("misaligned critic_h_out", dict(rover={"critic_h_out": 4}), "state output"),
    ("missing critic_h_out, value only", dict(rover={"critic_h_out": None}, flags=VO), "state output"),
    ("missing actor_h_out", dict(rover={"actor_h_out": None}), "state output"), ("misaligned actor_h_out", dict(rover={"actor_h_out": 8}), "state output"),
    ("misaligned actor_h_in", dict(rover={"actor_h_in": 4}), "state input"), ("misaligned critic_h_in", dict(rover={"critic_h_in": 4}), "state input"),
]


def test_c_entry_refusals_come_before_any_launch_in_the_shared_entrys_order():
    pol, _, x, _, _, _, _ = _setup(S33)
    for what, kw, word in REFUSALS:
        rc, msg, untouched = _refused(pol, x, **kw)
        assert rc == abi.HNS_ERR_INVALID_ARG, what
        assert msg.startswith("hns_policy_forward_rnn_agents: ") and word in msg, (what, msg)
        assert untouched, what
    # the first failing check names itself: the packed image before the GRU image before the flags before the outputs before the states
    assert "packed image / io" in _refused(pol, x, packed=False, rnn_packed=False)[1]
    assert "GRU image" in _refused(pol, x, rnn_packed=False, flags=4)[1]
    assert "flag" in _refused(pol, x, flags=4, over={"obs_self": None})[1]
    assert "observation" in _refused(pol, x, over={"obs_self": None, "value": None})[1]
    assert "value" in _refused(pol, x, over={"value": None}, rover={"critic_h_out": None})[1]
    # value only needs neither the actor's outputs and states nor the counter; the mode draws no noise
    rc, msg, _ = _refused(pol, x, flags=VO, over={"action": None, "log_prob": None}, rover={"actor_h_out": None, "actor_h_in": 4}, counter=False)
    assert rc == abi.HNS_OK, msg
    rc, msg, _ = _refused(pol, x, flags=DET, counter=False)
    assert rc == abi.HNS_OK, msg
    # the actor-only entry, hns_policy_act_rnn's order
    for what, kw, word in (("null packed image", dict(packed=False), "packed image"), ("8 agents", dict(shape=(35, 33, 8, 5)), "num_agents"),
                           ("null rnn image", dict(rnn_packed=False), "GRU image"), ("null rio", dict(rio=False), "rnn io"),
                           ("missing obs_self", dict(over={"obs_self": None}), "observation"), ("missing action", dict(over={"action": None}), "action"),
                           ("missing actor_h_out", dict(rover={"actor_h_out": None}), "state output"),
                           ("misaligned actor_h_in", dict(rover={"actor_h_in": 4}), "state input")):
        rc, msg, untouched = _refused(pol, x, entry="act", **kw)
        assert rc == abi.HNS_ERR_INVALID_ARG and msg.startswith("hns_policy_act_rnn_agents: ") and word in msg and untouched, (what, msg)
    assert "GRU image" in _refused(pol, x, entry="act", rnn_packed=False, over={"action": None})[1]
    # the pack
    lib, n = pol._lib, pol._gru_net(pol.actor_rnn)
    bad = abi.HNS_ERR_INVALID_ARG
    assert lib.hns_policy_rnn_pack_agents(C.byref(n), C.byref(n), 8, pol.rnn_packed.data_ptr(), None) == bad and "num_agents" in lib.hns_last_error().decode()
    assert lib.hns_policy_rnn_pack_agents(C.byref(n), C.byref(n), 3, pol.rnn_packed.data_ptr() + 4, None) == bad
    assert lib.hns_policy_rnn_pack_agents(None, C.byref(n), 3, pol.rnn_packed.data_ptr(), None) == bad
    n.ln_b = None
    assert lib.hns_policy_rnn_pack_agents(C.byref(n), C.byref(n), 3, pol.rnn_packed.data_ptr(), None) == bad and "GRU parameter" in lib.hns_last_error().decode()


# ---- 7. the collector -------------------------------------------------------------------------------------------------------------------
N_ENVS, T_STEPS, SEQ, EPISODE = 64, 8, 4, 6


def _make_env(episode, seed=0):
    from hns_amd.env import HideAndSeek
    torch.manual_seed(seed + 100)                                # the predictor's initial weights come from the global generator
    cfg = config.make_cfg({"num_agents": 3, "env": {"num_envs": N_ENVS, "max_episode_length": episode}}, algo={"use_TP_net": 1})
    env = HideAndSeek(cfg, headless=True)
    env.set_seed(seed)
    return env


def _env_policy(env, seed):
    D = abi.self_dim(env.num_targets) + (3 * env.tp_future_step * env.num_targets if env.use_TP_net else 0)
    actors, critic = P.random_parameters_per_agent(D, env.num_agents, seed=seed)
    actors.update(P.random_rnn_parameters_per_agent(env.num_agents, seed + 1))
    critic.update(P.random_rnn_parameters(seed + 2))
    actors["act_dist.fc_mean.weight"] = actors["act_dist.fc_mean.weight"] * 30.0  # actions of order 0.3: the drones move
    return P.PerAgentRecurrentDevicePolicy(actors, critic, device=env.device, seed=seed)


def _hand_collect(env, pol, T, L):
    """What a user writes without the collector: a full reset, clones into lists, the states carried out of place, the flags handed over on
    every step, `done` read back on every step."""
    n, a = env.num_envs, env.num_agents
    cur = env.reset()
    ha, hc = torch.zeros(n, a, 128, device="cuda"), torch.zeros(n, a, 128, device="cuda")
    flags = torch.ones(n, 1, dtype=torch.bool, device="cuda")
    buf, seg = {}, {"actor_rnn_state": [], "critic_rnn_state": []}
    for t in range(T):
        obs = cur[("agents", "observation")]
        xs, xo, xc = obs["state_self"], obs.get("state_others", None), obs["cylinders"]
        if t % L == 0:
            seg["actor_rnn_state"].append(ha.clone())
            seg["critic_rnn_state"].append(hc.clone())
        out = pol.forward(xs, xo, xc, actor_state=ha, critic_state=hc, is_init=flags)
        step = {"obs_self": xs, "obs_others": xo, "obs_cylinders": xc, "action": out.action, "log_probs": out.log_prob, "state_value": out.value,
                "is_init": flags}
        for k, v in step.items():
            buf.setdefault(k, []).append(v.clone())
        ha, hc = out.actor_state, out.critic_state
        nxt = env.step(env.rand_step_input(out.action))["next"]
        done = nxt["done"]
        post = {"reward": nxt[("agents", "reward")], "done": done, **{k: nxt[("agents", "TP", k)] for k in collector.TP_KEYS}}
        for k, v in post.items():
            buf.setdefault(k, []).append(v.clone())
        if t == T - 1:
            nobs = nxt[("agents", "observation")]
            last = {"obs_self": nobs["state_self"].clone(), "obs_others": nobs["state_others"].clone(), "obs_cylinders": nobs["cylinders"].clone(),
                    "critic_rnn_state": hc.clone(), "is_init": done.clone()}
        flags = done.clone()
        cur = env.reset(TensorDict({"_reset": done.clone()}, env.batch_size)) if bool(done.any()) else nxt
    return {k: torch.stack(v, 1) for k, v in buf.items()}, {k: torch.stack(v, 1) for k, v in seg.items()}, last


def test_the_collector_stores_what_a_hand_driven_loop_over_forward_stores():
    """64 envs, 3v1, predictor on, T = 8 in segments of 4, episodes of 6 steps (a boundary inside the rollout): storage, recurrent_kwargs()
    and last bit for bit; DeviceCollector is the one the shared recurrent policy runs under, unchanged."""
    envs = [_make_env(EPISODE) for _ in range(2)]
    try:
        pols = [_env_policy(e, 5) for e in envs]
        col = collector.DeviceCollector(envs[0], pols[0], T_STEPS, rnn_seq_len=SEQ)
        assert col.recurrent
        st = col.collect()
        data, seg, last = _hand_collect(envs[1], pols[1], T_STEPS, SEQ)
        for part, got, want in (("data", st.data, data), ("segments", st.segments, seg), ("last", st.last, last)):
            assert set(got) == set(want), (part, set(got) ^ set(want))
            for k in want:
                assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (part, k)
        rk = st.recurrent_kwargs()
        assert rk["actor_rnn_state"].shape == (N_ENVS, T_STEPS // SEQ, 3, 128) and rk["rnn_seq_len"] == SEQ
        assert torch.equal(rk["is_init"], data["is_init"]) and torch.equal(rk["last_critic_rnn_state"], last["critic_rnn_state"])
        assert torch.equal(rk["last_is_init"], last["is_init"]) and torch.equal(rk["critic_rnn_state"], seg["critic_rnn_state"])
        steps = torch.arange(1, T_STEPS + 1, device="cuda")
        assert torch.equal(data["done"], (steps % EPISODE == 0).view(1, -1, 1).expand(N_ENVS, -1, 1))        # the boundary inside the rollout
        assert bool(data["is_init"][:, 0].all()) and bool(data["is_init"][:, EPISODE].all()) and int(data["is_init"].sum()) == 2 * N_ENVS
        assert float(seg["actor_rnn_state"][:, 1].abs().max()) > 0 and int(pols[0].counter) == T_STEPS
        assert "tp" in st.learner_kwargs()
    finally:
        for e in envs:
            e.close()


# ---- 8. the evaluator -------------------------------------------------------------------------------------------------------------------
def test_evaluate_equals_the_stateful_hand_loop_with_one_action_and_one_state_tensor():
    L = 6
    env, hand = _make_env(L), _make_env(L)
    try:
        pol = _env_policy(env, 8)
        counter = pol.counter.clone()
        calls = []
        act_step = pol.act_step

        def recording(*a, **kw):
            action, state = act_step(*a, **kw)
            calls.append((kw.get("state"), kw.get("out"), kw.get("out_state"), action, state))
            return action, state
        pol.act_step = recording
        ev = evaluator.DeviceEvaluator(env, pol)
        info = ev.evaluate(seed=3)
        pol.act_step = act_step
        assert (ev.steps, ev.done_reads, ev.launches) == (L, 1, 1) and torch.equal(pol.counter, counter)
        assert len(calls) == L and calls[0][0] is None and calls[0][1] is None
        action, state = calls[0][3], calls[0][4]
        assert tuple(state.shape) == (N_ENVS, 3, 128) and tuple(action.shape) == (N_ENVS, 3, 4)
        for s_in, out, s_out, a, s in calls[1:]:                 # ONE action tensor, ONE state tensor, in place
            assert s_in is state and s_out is state and out is action and a is action and s is state
        ERC.hand_loop(hand, pol, 3, hand.rand_step_input, stateful=True)
        assert set(info) == {"eval/stats." + k for k in abi.STAT_NAMES}
        for k in abi.STAT_NAMES:
            assert LC.bits_equal(ev.stats[k], hand.stats[k].reshape(-1)), k
            want, _, _ = evaluator.stat_means([hand.stats[k]], None)
            assert np.array_equal(np.array([info["eval/stats." + k]], np.float32), want, equal_nan=True), k
    finally:
        env.close()
        hand.close()


# ---- 9. the example script ---------------------------------------------------------------------------------------------------------------
def test_the_example_collects_evaluates_and_reloads_its_checkpoint():
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "per_agent_recurrent.py")
    run = subprocess.run([sys.executable, script, "--envs", "64", "--steps", "8", "--seq-len", "4", "--episode", "6"], capture_output=True, text=True,
                         timeout=240)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "3 recurrent actors, stacked: rnn.cell.weight_hh (3, 384, 128)" in run.stdout and "eval: eval/stats.success" in run.stdout
    assert "are bit for bit the first's" in run.stdout and "the agents' actions differ" in run.stdout
    assert "is_init (64, 8, 1) (128 set)" in run.stdout                               # the full reset and the boundary at step 6


def test_report_ratios():
    print("recurrent per-agent gate ratios:", {k: round(v, 2) for k, v in RATIOS.items()})
