"""hns_policy_forward_rnn and hns_policy_act_rnn on an MI355X at their tile, flag, state and numerical edges (test_hip_policy_rnn.py and
test_hip_evaluator_rnn.py hold the kernels to the gate and to each other at 3, 33, 5 and 21 rows; the cases here are policy_rnn_cases.py's,
and test_policy_rnn.py shows on the CPU that each of them can fail).

Accuracy gate (test_hip_policy_rnn.py's rule): per output, e_hip <= 8 max(e_32, 2^-24 max|ref_64|), errors as max-abs against the fp64
restatement (tests/policy_rnn_reference.py), at every step of a chain in which the kernel's own h_out feeds its next call.  Everything else
is bit for bit: guard rows around every output of the C calls, the three call forms and the actor-only pass against each other, flags
against zeroed states at tiles that start inside an env, in place against out of place, a tile's envs alone against the big call.

Worst ratio per group over all outputs and steps, measured on an MI355X (RATIOS, printed by the last test): sweep 2.08, full tiles 1.63,
straddle 1.45; flat_tokens 6.00 (value, step 2; the non-recurrent gate's 3.86 behind a GRU), saturated_softmax 5.25, large_obs 1.30,
saturated_gates 5.71, large_state 1.09, carry 1.88 (log_prob; both states 0: exact), near_flat_norm 1.08; the long chain 1.65 over its first
5 steps and 1.79 over all 64 (at step 7: no drift).  A library built with the flag read at env row0 / A + r / A passes all of
test_hip_policy_rnn.py and test_hip_evaluator_rnn.py and fails 29 of the 88 tests here, the chains test_policy_rnn.py predicts: 15 of the
sweep, the 96-row full tile, every straddle and row-independence case with flags in the cut, every edge."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import policy_rnn_cases as PC
import policy_rnn_reference as RR
from hns_amd import abi
from hns_amd import policy as P

pytestmark = pytest.mark.gpu

BAR = RR.BAR
RATIOS = {}
PATTERN = 0x7FA5C3E1                                             # the bits of a NaN: a live word left unwritten is not finite
GUARD_FRONT, GUARD_BEHIND = 4, 64                                # rows; four rows of any output keep the 16-byte alignment of the states
WIDTH = {"action": 4, "log_prob": 1, "loc": 4, "value": 1, "actor_h_out": 128, "critic_h_out": 128}
ACTOR_OUTPUTS = ("action", "log_prob", "loc", "actor_h_out")
NAMES = {"loc": "loc", "log_prob": "log_prob", "value": "value", "actor_state": "actor_h_out", "critic_state": "critic_h_out"}
VO, DET = abi.HNS_POLICY_VALUE_ONLY, abi.HNS_POLICY_DETERMINISTIC


def _cuda(x):
    return torch.as_tensor(np.asarray(x)).cuda() if x is not None else None


def _obs_dev(obs):
    return _cuda(obs["state_self"]), _cuda(obs.get("state_others")), _cuda(obs["cylinders"])


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _setup(tag):
    """(policy, device observations per step, eps per step, flags per step (uint8), the two start states) of a chain of policy_rnn_cases."""
    actor, critic, obs, eps, flags, ha, hc = PC.case(tag)
    dev = lambda p: {k: _cuda(v) for k, v in p.items()}
    pol = P.RecurrentDevicePolicy(dev(actor), dev(critic), seed=11)
    return pol, [_obs_dev(o) for o in obs], [_cuda(e) for e in eps], [_cuda(f).view(torch.uint8) for f in flags], _cuda(ha), _cuda(hc)


def _gate(group, tag, t, got, refs):
    """The gate on one step's outputs ({name: tensor}); returns the step's worst ratio and records the group's."""
    ratios = RR.gate_ratios({n: got[n].cpu().double().numpy() for n in RR.OUTPUTS}, *refs)
    print(f"  {tag} step {t}: " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    for name, ratio in ratios.items():
        assert ratio <= BAR, f"{tag} step {t} {name}: ratio {ratio:.2f} > {BAR}"
    worst = max(ratios.values())
    RATIOS[group] = max(RATIOS.get(group, 0.0), worst)
    return worst


# ---- the C calls with caller buffers inside guard rows ---------------------------------------------------------------------------------
class Guarded:
    """`rows` rows of `width` fp32 words inside a pattern-filled buffer: GUARD_FRONT rows in front of them, GUARD_BEHIND behind."""

    def __init__(self, rows, width):
        self.lo, self.hi = GUARD_FRONT * width, (GUARD_FRONT + rows) * width
        self.raw = torch.full((self.hi + GUARD_BEHIND * width,), PATTERN, dtype=torch.int32, device="cuda")
        self.ptr = self.raw.data_ptr() + 4 * self.lo
        self.width = width

    def guards_intact(self):
        return bool((self.raw[:self.lo] == PATTERN).all()) and bool((self.raw[self.hi:] == PATTERN).all())

    def untouched(self):
        return bool((self.raw == PATTERN).all())

    def written(self):
        live = self.raw[self.lo:self.hi]
        return bool((live != PATTERN).all()) and bool(torch.isfinite(live.view(torch.float32)).all())

    def values(self, E, A):
        return self.raw[self.lo:self.hi].view(torch.float32).view(E, A, self.width)


def _call(pol, x, ha, hc, flags, eps, mode):
    """One C call with every output pointer set and inside guard rows.  mode: "sample" (the caller's eps), "det", "value_only" (all buffers
    non-NULL all the same) or "act" (hns_policy_act_rnn).  -> {output name: Guarded}, (E, A); the call counter must not move in any of them."""
    pol.refresh()
    xs, xo, xc, io = pol._io(x[0].squeeze(2), x[1], x[2])
    E, A, K = xs.shape[0], xs.shape[1], xc.shape[2]
    bufs = {n: Guarded(E * A, w) for n, w in WIDTH.items()}
    io.action, io.log_prob, io.loc, io.value = (bufs[n].ptr for n in ("action", "log_prob", "loc", "value"))
    io.eps = eps.data_ptr() if mode == "sample" else None
    rio = abi.HnsPolicyRnnIo()
    rio.actor_h_in, rio.critic_h_in = ha.data_ptr(), hc.data_ptr()
    rio.actor_h_out, rio.critic_h_out = bufs["actor_h_out"].ptr, bufs["critic_h_out"].ptr
    rio.is_init = flags.data_ptr() if flags is not None else None
    assert all(b.ptr % 16 == 0 for b in bufs.values())
    c0 = int(pol.counter)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if mode == "act":
        rc = pol._lib.hns_policy_act_rnn(pol.packed.data_ptr(), pol.rnn_packed.data_ptr(), pol.self_dim, E, A, K, C.byref(io), C.byref(rio), st)
    else:
        bits = {"sample": 0, "det": DET, "value_only": VO}[mode]
        rc = pol._lib.hns_policy_forward_rnn(pol.packed.data_ptr(), pol.rnn_packed.data_ptr(), pol.self_dim, E, A, K, C.byref(io), C.byref(rio), bits,
                                             pol.seed, pol.counter.data_ptr(), st)
    assert rc == abi.HNS_OK, pol._lib.hns_last_error()
    torch.cuda.synchronize()
    assert int(pol.counter) == c0
    return bufs, (E, A)


WRITES = {"sample": tuple(WIDTH), "det": tuple(WIDTH), "value_only": ("value", "critic_h_out"), "act": ("action", "actor_h_out")}


def _check_buffers(bufs, mode, where):
    """Every guard word keeps its bits, every live word of what the call writes is written, everything else is entirely untouched."""
    for name, b in bufs.items():
        if name in WRITES[mode]:
            assert b.guards_intact(), f"{where} {mode}: a guard row of {name} was written"
            assert b.written(), f"{where} {mode}: a live word of {name} was not written (or is not finite)"
        else:
            assert b.untouched(), f"{where} {mode}: {name} was written"


def _run_chain(tag, modes):
    """The chain `tag` through the C calls: at every step each of `modes` from the same inputs; the FIRST mode's states feed the next step.
    -> [{mode: {output name: [E, A, width] tensor}}] per step (buffers checked)."""
    pol, obs, eps, flags, ha, hc = _setup(tag)
    steps = []
    for t in range(len(obs)):
        step = {}
        for mode in modes:
            bufs, (E, A) = _call(pol, obs[t], ha, hc, flags[t], eps[t], mode)
            _check_buffers(bufs, mode, f"{tag} step {t}")
            step[mode] = {n: b.values(E, A) for n, b in bufs.items()}
        ha, hc = step[modes[0]]["actor_h_out"].clone(), step[modes[0]]["critic_h_out"].clone()
        steps.append(step)
    return steps


TILE_TAGS = PC.SWEEP_TAGS + PC.FULL_TAGS


# ---- 1, 3. the seeded sweep and the full tiles -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TILE_TAGS)
def test_every_tail_length_passes_the_gate_inside_guard_rows_in_all_three_call_forms(tag):
    """A 2-step chain (the kernel's own states feed step 2, where half of the envs are flagged) at E A mod 32 = 0 .. 31 and at 32, 64 and 96
    rows: sampling through the gate at both steps; deterministic: action == loc, everything but log_prob the sampling call's bits;
    value-only: the actor's four outputs untouched, value and the critic's state the sampling call's bits."""
    actor = PC.case(tag)[0]
    refs = PC.references(tag)
    for t, step in enumerate(_run_chain(tag, ("sample", "det", "value_only"))):
        s, d, v = step["sample"], step["det"], step["value_only"]
        _gate("full tiles" if tag in PC.FULL_TAGS else "sweep", tag, t, {n: s[b] for n, b in NAMES.items()}, refs[t])
        for n in ("loc", "value", "actor_h_out", "critic_h_out"):
            assert _bits(d[n], s[n]), (tag, t, n)
        assert _bits(d["action"], d["loc"]) and not _bits(s["action"], s["loc"])
        lp64, lp32 = (RR.mode_log_prob(actor, d["log_prob"].shape[:2], dt).double().numpy() for dt in (torch.float64, torch.float32))
        e = np.abs(d["log_prob"].cpu().double().numpy() - lp64).max()
        assert e <= BAR * max(np.abs(lp32 - lp64).max(), 2.0 ** -24 * np.abs(lp64).max()), (tag, t, e)
        assert _bits(v["value"], s["value"]) and _bits(v["critic_h_out"], s["critic_h_out"]), (tag, t)


# ---- 2, 3. the actor-only pass over the same chains ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TILE_TAGS)
def test_act_rnn_is_the_deterministic_forwards_actor_half_at_every_tail_length(tag):
    """hns_policy_act_rnn inside the same guard rows: action and actor_h_out the deterministic forward's bits; log_prob, loc, value, the
    critic's state and the call counter untouched (all of them non-NULL)."""
    for t, step in enumerate(_run_chain(tag, ("det", "act"))):
        assert _bits(step["act"]["action"], step["det"]["action"]), (tag, t)
        assert _bits(step["act"]["actor_h_out"], step["det"]["actor_h_out"]), (tag, t)


# ---- 4. flags at tiles that do not start on an env boundary ----------------------------------------------------------------------------
def _flag_sets(E, A):
    split = PC.straddling_envs(E, A)
    return {"straddlers": split, "complement": [e for e in range(E) if e not in split], "one below": sorted({e - 1 for e in split})}


@pytest.mark.parametrize("shape", PC.STRADDLE_SHAPES, ids=PC.shape_tag)
def test_a_flag_holds_for_its_env_and_no_other_where_tiles_start_inside_an_env(shape):
    """Exactly the straddling envs flagged, exactly the others, exactly the envs one below a straddler: each call is bit for bit the call with
    those envs' states zeroed and no flags, the unflagged envs' rows are the unflagged call's, and NaN in a flagged env's h_in reaches no
    output — for the forward, for value-only and for act_step.  The straddlers' set goes through the fp64 gate as well."""
    tag = "straddle-" + PC.shape_tag(shape)
    pol, obs, eps, _, ha, hc = _setup(tag)
    x, e = obs[0], eps[0]
    E, A = ha.shape[:2]
    plain = pol.forward(*x, actor_state=ha, critic_state=hc, eps=e)
    for what, envs in _flag_sets(E, A).items():
        f = torch.zeros(E, dtype=torch.bool, device="cuda")
        f[envs] = True
        assert 0 < len(envs) < E
        za, zc, na, nc = ha.clone(), hc.clone(), ha.clone(), hc.clone()
        za[f], zc[f] = 0, 0
        na[f], nc[f] = float("nan"), float("nan")                # a flagged row's h_in is not read
        got = pol.forward(*x, actor_state=na, critic_state=nc, is_init=f, eps=e)
        want = pol.forward(*x, actor_state=za, critic_state=zc, eps=e)
        for n in RR.OUTPUTS + ("action",):
            a, b, c = getattr(got, n), getattr(want, n), getattr(plain, n)
            assert bool(torch.isfinite(a).all()), (what, n)
            assert _bits(a, b), (what, n)
            assert _bits(a[~f], c[~f]), (what, n)
            if n != "log_prob":                                  # (with the caller's eps, action - loc = scale eps whatever loc is)
                differ = (a != c).flatten(1).any(1)
                assert bool(differ[f].all()), (what, n)          # ... and every flagged env's rows are not
        vo = pol.forward(*x, critic_state=nc, is_init=f, value_only=True)
        assert _bits(vo.value, got.value) and _bits(vo.critic_state, got.critic_state), what
        action, state = pol.act_step(*x, state=na, is_init=f)
        assert _bits(action, got.loc) and _bits(state, got.actor_state), what
        if what == "straddlers":
            assert np.array_equal(f.cpu().numpy(), PC.case(tag)[4][0])
            _gate("straddle", tag, 0, {n: getattr(got, n) for n in RR.OUTPUTS}, PC.references(tag)[0])


# ---- 5. in place across tiles ----------------------------------------------------------------------------------------------------------
IN_PLACE_TAGS = ["straddle-" + PC.shape_tag(PC.STRADDLE_SHAPES[-1]), next(t for s, t in zip(PC.SWEEP_SEEDS, PC.SWEEP_TAGS) if PC.tiles_of(PC.sweep_shape(s)) >= 4)]


@pytest.mark.parametrize("tag", IN_PLACE_TAGS)
def test_in_place_states_give_the_out_of_place_bits_over_many_tiles(tag):
    """Three steps with out_states aliasing the input states (h_out == h_in: a workgroup that touched another's rows would read a state
    already overwritten) against the out-of-place chain, for the forward and for act_step.  The chain's observations and flags in turn."""
    pol, obs, eps, flags, ha, hc = _setup(tag)
    assert -(-ha.shape[0] * ha.shape[1] // 32) >= 4
    ia, ic, sa = ha.clone(), hc.clone(), ha.clone()
    oa, oc = ha, hc
    for t in range(3):
        x, e, f = obs[t % len(obs)], eps[t % len(obs)], flags[-1] if t == 1 else None
        want = pol.forward(*x, actor_state=oa, critic_state=oc, is_init=f, eps=e)
        got = pol.forward(*x, actor_state=ia, critic_state=ic, is_init=f, eps=e, out_states=(ia, ic))
        assert got.actor_state is ia and got.critic_state is ic
        for n in RR.OUTPUTS + ("action",):
            assert _bits(getattr(got, n), getattr(want, n)), (tag, t, n)
        action, state = pol.act_step(*x, state=sa, is_init=f, out_state=sa)
        assert state is sa and _bits(action, want.loc) and _bits(sa, want.actor_state), (tag, t)
        oa, oc = want.actor_state, want.critic_state
    assert not _bits(oa, ha)


# ---- 6. row independence beyond the second tile ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PC.STRADDLE_SHAPES[1:], ids=PC.shape_tag)
def test_the_envs_of_a_later_tile_alone_give_the_bits_they_have_in_the_big_call(shape):
    """Every env with a row in tile 3 (rows 96 .. 127) of a call of seven to nine tiles, run alone with the same eps, states and flags: other
    tile positions, the same bits."""
    tag = "straddle-" + PC.shape_tag(shape)
    pol, obs, eps, flags, ha, hc = _setup(tag)
    E, A = ha.shape[:2]
    assert -(-E * A // 32) >= 5
    envs = [e for e in range(E) if e * A < 128 and e * A + A > 96]
    lo, hi = envs[0] + (envs[0] * A % 32 == 0), envs[-1] + 1      # (not from the tile's first row: the rows change their place in the tile)
    assert lo * A % 32 != 0 and hi - lo >= 4 and bool(flags[0][lo:hi].any()) and not bool(flags[0][lo:hi].all())
    x, f = obs[0], flags[0]
    big = pol.forward(*x, actor_state=ha, critic_state=hc, is_init=f, eps=eps[0])
    cut = lambda t: t[lo:hi].contiguous() if t is not None else None
    small = pol.forward(*(cut(t) for t in x), actor_state=cut(ha), critic_state=cut(hc), is_init=cut(f), eps=cut(eps[0]))
    for n in RR.OUTPUTS + ("action",):
        assert _bits(getattr(small, n), getattr(big, n)[lo:hi]), n
    action, state = pol.act_step(*(cut(t) for t in x), state=cut(ha), is_init=cut(f))
    assert _bits(action, big.loc[lo:hi]) and _bits(state, big.actor_state[lo:hi])


# ---- 7, 8. chains through the class ----------------------------------------------------------------------------------------------------
def _chain_gate(group, tag, act=False):
    """The gate at every step of the chain `tag`, the device's own states feeding its next step (the fp64 and fp32 chains feed themselves);
    act: act_step's own chain beside it, bit for bit the deterministic forward's.  -> (outputs per step, worst ratio per step)."""
    pol, obs, eps, flags, ha, hc = _setup(tag)
    refs = PC.references(tag)
    outs, worst, sa = [], [], ha
    for t in range(len(obs)):
        out = pol.forward(*obs[t], actor_state=ha, critic_state=hc, is_init=flags[t], eps=eps[t])
        for n in RR.OUTPUTS + ("action",):
            assert bool(torch.isfinite(getattr(out, n)).all()), (tag, t, n)
        worst.append(_gate(group, tag, t, {n: getattr(out, n) for n in RR.OUTPUTS}, refs[t]))
        if act:
            det = pol.forward(*obs[t], actor_state=ha, critic_state=hc, is_init=flags[t], deterministic=True)
            action, sa = pol.act_step(*obs[t], state=sa, is_init=flags[t])
            assert _bits(det.loc, out.loc) and _bits(action, det.action) and _bits(sa, det.actor_state), (tag, t)
        outs.append((ha, hc, out))
        ha, hc = out.actor_state, out.critic_state
    return outs, worst


@pytest.mark.parametrize("name", PC.EDGES)
def test_numerical_edges_pass_the_gate_along_a_self_fed_chain(name):
    """The encoder's three edges behind a GRU, saturated gates, large states, an update gate that is exactly one and a nearly flat norm: three
    steps, every output finite.  carry (and near_flat_norm, which is carry): the states of unflagged rows come out bit for bit as they went
    in, those of flagged rows are all zeros."""
    outs, _ = _chain_gate(name, name)
    if name in ("carry", "near_flat_norm"):
        flags = _setup(name)[3]
        for t, (ha, hc, out) in enumerate(outs):
            f = flags[t].bool()
            for h_in, h_out in ((ha, out.actor_state), (hc, out.critic_state)):
                assert _bits(h_out[~f], h_in[~f]), (name, t)
                assert bool((h_out[f] == 0).all()), (name, t)    # (1 - 1) n + 1 * 0
        assert bool(flags[1].any())


def test_the_long_chain_passes_the_gate_at_each_of_its_64_steps():
    """64 steps at 33 rows (a segment is 16, the other chains 5) with flags around the segment boundary, and act_step's chain beside it."""
    _, worst = _chain_gate("long chain", "long-%d" % PC.LONG_STEPS, act=True)
    assert len(worst) == 64
    RATIOS["long chain, first 5 steps"] = max(worst[:5])
    print(f"  long chain: worst ratio {max(worst[:5]):.2f} over the first 5 steps, {max(worst):.2f} over all 64 (step {int(np.argmax(worst))})")


def test_report_ratios():
    print("recurrent policy edge ratios:", {k: round(v, 2) for k, v in RATIOS.items()})
