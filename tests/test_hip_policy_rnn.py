"""hns_policy_forward_rnn (through hns_amd.policy.RecurrentDevicePolicy and through the C ABI) and the collector's rnn state on an MI355X.

Accuracy gate (test_hip_policy.py's rule): per output, e_hip <= 8 max(e_32, 2^-24 max|ref_64|), errors as max-abs against the fp64
restatement (tests/policy_rnn_reference.py), e_32 the error of the same statements in CPU torch fp32 — for loc, log_prob (eps supplied),
value and both states, at EVERY step of a chain in which the kernel's own h_out feeds its next call (the fp64 and fp32 chains feed
themselves): the golden cases, random batches at the shapes where the tile can go wrong, observations read through strided views.
Exact properties, refusals, and the collector against a hand-driven loop (copy_ stores, an explicit state carry, flags on every step) are
bit for bit.  Worst ratio per case over all outputs and steps, measured on an MI355X (RATIOS, printed by the last test): goldens 1.48 / 1.76,
random e1a3k5d35 2.08, e11a3k5d35 1.25, e5a1k5d20 1.99, e3a7k16d96 1.40, strided views 1.52; over a stored segment the ops' log_prob 1.21 and
value 1.02, the collected (fused) ones 1.00 and 0.83, largest |log_prob_op - log_prob_fused| 9.5e-7.

The tile, flag, guard-row and numerical edges of the same kernels (more than two tiles, every tail length, tiles that start inside an env,
guard rows around every output, saturated gates, a 64-step chain) are test_hip_policy_rnn_edges.py's."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import policy_reference as R
import policy_rnn_cases as PC
import policy_rnn_reference as RR
from hns_amd import abi, collector, config, encoder, rnn
from hns_amd import policy as P
from hns_amd.tensordict_shim import TensorDict

pytestmark = pytest.mark.gpu

BAR = RR.BAR
RATIOS = {}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (E, A, K, D): three rows of a 32-row tile; 33 rows (a second tile with one live row); no state_others; every limit at its maximum — and
# their chains' generator, shared with the CPU emulation of test_policy_rnn.py
SHAPES, STEPS, _random_chain = PC.SHAPES, PC.STEPS, PC.random_chain


def _dev(d):
    return {k: torch.as_tensor(np.asarray(v)).cuda() for k, v in d.items()}


def _obs_dev(obs):
    return (torch.as_tensor(obs["state_self"]).cuda(), torch.as_tensor(obs["state_others"]).cuda() if "state_others" in obs else None,
            torch.as_tensor(obs["cylinders"]).cuda())


def _cuda(x):
    return torch.as_tensor(np.asarray(x)).cuda() if x is not None else None


def _policy(actor, critic, seed=0):
    return P.RecurrentDevicePolicy(_dev(actor), _dev(critic), seed=seed)


def chain_gate(tag, actor, critic, obs, eps, flags, ha, hc, view=None):
    """The gate at every step of the chain; returns the kernel's outputs per step.  `view`: maps the device observations to what the policy is
    handed (strided views)."""
    pol = _policy(actor, critic)
    h_hip, h64, h32 = (_cuda(ha), _cuda(hc)), (ha, hc), (ha, hc)
    worst, outs = 0.0, []
    for t in range(len(obs)):
        x = _obs_dev(obs[t])
        out = pol.forward(*(view(x) if view else x), actor_state=h_hip[0], critic_state=h_hip[1], is_init=_cuda(flags[t]), eps=_cuda(eps[t]))
        got = {n: getattr(out, n).cpu().double().numpy() for n in RR.OUTPUTS}
        r64 = RR.forward(actor, critic, obs[t], h64[0], h64[1], flags[t], eps[t], torch.float64)
        r32 = RR.forward(actor, critic, obs[t], h32[0], h32[1], flags[t], eps[t], torch.float32)
        ratios = RR.gate_ratios(got, {k: v.numpy() for k, v in r64.items()}, {k: v.double().numpy() for k, v in r32.items()})
        print(f"  {tag} step {t}: " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
        for name, ratio in ratios.items():
            assert ratio <= BAR, f"{tag} step {t} {name}: ratio {ratio:.2f} > {BAR}"
        worst = max(worst, *ratios.values())
        h_hip = (out.actor_state, out.critic_state)
        h64, h32 = (r64["actor_state"], r64["critic_state"]), (r32["actor_state"], r32["critic_state"])
        outs.append(out)
    RATIOS[tag] = worst
    return outs


@pytest.fixture(scope="module")
def goldens():
    return tuple(np.load(os.path.join(GOLDEN, n)) for n in ("g_policy.npz", "g_gru.npz", "g_policy_rnn.npz"))


# ---- 1. the accuracy gate -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", RR.CASES)
def test_golden_chains_pass_the_fp64_gate_at_every_step(goldens, tag):
    gp, gg, z = goldens
    actor, critic = RR.golden_params(gp, gg, tag)
    case = RR.golden_case(z, tag)
    T = int(case["shape"][4])
    outs = chain_gate(tag, actor, critic, [RR.step_obs(case, t) for t in range(T)], list(case["eps"]), list(case["is_init"]),
                      case["h0:actor"], case["h0:critic"])
    for t, out in enumerate(outs):                               # and the reference's own numbers, at the goldens' 1e-5
        for name in ("loc", "action", "log_prob", "value", "actor_state", "critic_state"):
            assert float(np.abs(getattr(out, name).cpu().numpy() - case[name][t]).max()) <= 1e-5, (t, name)


@pytest.mark.parametrize("shape", SHAPES, ids=["e%da%dk%dd%d" % s for s in SHAPES])
def test_random_chains_pass_the_fp64_gate_at_every_step(shape):
    E, A, K, D = shape
    actor, critic = RR.random_net(D, A, 300 + E + A)
    chain_gate("random-e%da%dk%dd%d" % shape, actor, critic, *_random_chain(E, A, K, D, 400 + E))


def _embed(x, t_total, t, offset):
    """x [E, ...] as the view [:, t] of a NaN-filled [E, t_total, ...] parent with one more element in every trailing dimension, behind a
    storage offset: leading strides that are not the products of the inner extents, NaN wherever x is not."""
    shape = (x.shape[0], t_total) + tuple(s + 1 for s in x.shape[1:])
    flat = torch.full((offset + int(np.prod(shape)),), float("nan"), device="cuda")
    view = flat[offset:].view(shape)[:, t]
    for dim, s in enumerate(x.shape[1:], start=1):
        view = view.narrow(dim, 0, s)
    view.copy_(x)
    assert not view.is_contiguous() and view.stride(-1) == 1
    return view


def test_strided_observations_pass_the_gate_and_give_the_contiguous_bits():
    E, A, K, D = 11, 3, 5, 35
    actor, critic = RR.random_net(D, A, 501)
    chain = _random_chain(E, A, K, D, 502)
    view = lambda x: (_embed(x[0], 3, 1, 5), _embed(x[1], 3, 2, 3), _embed(x[2], 4, 2, 7))
    strided = chain_gate("strided", actor, critic, *chain, view=view)
    plain = chain_gate("strided-contiguous", actor, critic, *chain)
    for a, b in zip(strided, plain):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ---- 2. exact properties --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case11():
    E, A, K, D = 11, 3, 5, 35
    actor, critic = RR.random_net(D, A, 601)
    obs, eps = R.random_obs(E, A, K, D, 602)
    ha, hc = RR.random_states(E, A, 603)
    flags = np.zeros(E, bool)
    flags[[1, 4, 10]] = True
    return _policy(actor, critic, seed=77), _obs_dev(obs), _cuda(eps), _cuda(ha), _cuda(hc), _cuda(flags)


def _same(a, b, names=RR.OUTPUTS + ("action",)):
    for n in names:
        x, y = getattr(a, n), getattr(b, n)
        assert torch.isfinite(x).all() and torch.equal(x, y), n


def test_the_same_inputs_give_the_same_bits(case11):
    pol, x, e, ha, hc, f = case11
    _same(pol.forward(*x, actor_state=ha, critic_state=hc, is_init=f, eps=e), pol.forward(*x, actor_state=ha, critic_state=hc, is_init=f, eps=e))


def test_rows_do_not_depend_on_the_other_rows_of_the_call(case11):
    pol, x, e, ha, hc, f = case11
    full = pol.forward(*x, actor_state=ha, critic_state=hc, is_init=f, eps=e)
    part = pol.forward(*(t[:4] for t in x), actor_state=ha[:4].contiguous(), critic_state=hc[:4].contiguous(), is_init=f[:4], eps=e[:4])
    for n in RR.OUTPUTS + ("action",):
        assert torch.equal(getattr(full, n)[:4], getattr(part, n)), n


def test_is_init_is_a_zeroed_state_for_its_env_and_nothing_for_the_others(case11):
    pol, x, e, ha, hc, f = case11
    got = pol.forward(*x, actor_state=ha, critic_state=hc, is_init=f, eps=e)
    za, zc = ha.clone(), hc.clone()
    za[f.bool()], zc[f.bool()] = 0, 0
    _same(got, pol.forward(*x, actor_state=za, critic_state=zc, eps=e))
    plain = pol.forward(*x, actor_state=ha, critic_state=hc, eps=e)
    for n in RR.OUTPUTS:
        a, b = getattr(got, n), getattr(plain, n)
        assert torch.equal(a[~f.bool()], b[~f.bool()]), n
        if n != "log_prob":                                      # (with the caller's eps, action - loc = scale eps whatever loc is)
            assert not torch.equal(a[f.bool()], b[f.bool()]), n
    _same(got, pol.forward(*x, actor_state=ha, critic_state=hc, is_init=f.to(torch.uint8).reshape(-1, 1), eps=e))          # uint8 [E, 1] flags


def test_a_null_state_is_a_state_of_zeros_and_in_place_is_out_of_place(case11):
    pol, x, e, ha, hc, f = case11
    _same(pol.forward(*x, eps=e), pol.forward(*x, actor_state=torch.zeros_like(ha), critic_state=torch.zeros_like(hc), eps=e))
    want = pol.forward(*x, actor_state=ha, critic_state=hc, is_init=f, eps=e)
    ia, ic = ha.clone(), hc.clone()
    got = pol.forward(*x, actor_state=ia, critic_state=ic, is_init=f, eps=e, out_states=(ia, ic))
    assert got.actor_state is ia and got.critic_state is ic
    _same(got, want)


def test_value_only_touches_the_critics_half_alone(case11):
    pol, x, e, ha, hc, f = case11
    want = pol.forward(*x, actor_state=ha, critic_state=hc, is_init=f, eps=e)
    E, A = ha.shape[:2]
    pol.refresh()
    xs, xo, xc, io = pol._io(x[0].squeeze(2), x[1], x[2])
    sent = lambda *s: torch.full(s, 12345.0, device="cuda")
    action, logp, loc, h_a, value, h_c = sent(E, A, 4), sent(E, A), sent(E, A, 4), sent(E, A, 128), sent(E, A), sent(E, A, 128)
    io.action, io.log_prob, io.loc, io.value = action.data_ptr(), logp.data_ptr(), loc.data_ptr(), value.data_ptr()
    rio = abi.HnsPolicyRnnIo()
    rio.actor_h_in = 16                                          # never read: an address that would fault
    rio.critic_h_in, rio.actor_h_out, rio.critic_h_out, rio.is_init = hc.data_ptr(), h_a.data_ptr(), h_c.data_ptr(), f.view(torch.uint8).data_ptr()
    c0 = int(pol.counter)
    for flags in (abi.HNS_POLICY_VALUE_ONLY, abi.HNS_POLICY_VALUE_ONLY | abi.HNS_POLICY_DETERMINISTIC):
        rc = pol._lib.hns_policy_forward_rnn(pol.packed.data_ptr(), pol.rnn_packed.data_ptr(), pol.self_dim, E, A, xc.shape[2], C.byref(io),
                                             C.byref(rio), flags, pol.seed, pol.counter.data_ptr(), None)
        assert rc == abi.HNS_OK, pol._lib.hns_last_error()
        torch.cuda.synchronize()
        for t in (action, logp, loc, h_a):
            assert bool((t == 12345.0).all())
        assert torch.equal(value.reshape(E, A, 1), want.value) and torch.equal(h_c, want.critic_state) and int(pol.counter) == c0
    vo = pol.forward(*x, critic_state=hc, is_init=f, value_only=True)
    assert vo.action is None and vo.actor_state is None and torch.equal(vo.value, want.value) and torch.equal(vo.critic_state, want.critic_state)


def test_modes_and_noise(case11):
    pol, x, e, ha, hc, f = case11
    kw = dict(actor_state=ha, critic_state=hc, is_init=f)
    out = pol.forward(*x, eps=e, **kw)
    det = pol.forward(*x, deterministic=True, **kw)
    assert torch.equal(det.action, det.loc) and torch.equal(det.loc, out.loc) and torch.equal(det.value, out.value)
    assert torch.equal(det.actor_state, out.actor_state)
    loc, act, scale = out.loc.cpu().numpy(), out.action.cpu().numpy(), pol.scale.cpu().numpy()
    assert np.array_equal(act, (loc + scale * e.cpu().numpy()).astype(np.float32))                # bit for bit: two fp32 roundings
    c0 = int(pol.counter)
    a1 = pol.forward(*x, **kw)
    assert int(pol.counter) == c0 + 1
    a2 = pol.forward(*x, **kw)
    assert int(pol.counter) == c0 + 2 and not torch.equal(a1.action, a2.action)
    assert torch.equal(a1.loc, a2.loc) and torch.equal(a1.critic_state, a2.critic_state)
    pol.counter.fill_(c0)
    assert torch.equal(pol.forward(*x, **kw).action, a1.action)
    # the noise of row r is that of the non-recurrent forward pass at the same seed, counter and row
    z = ((a1.action - a1.loc) / pol.scale).cpu().numpy().reshape(-1, 4)
    want = R.philox_normal(pol.seed, c0, z.shape[0], np.float32)
    assert np.abs(z - want).max() < 1e-3


def test_the_next_call_follows_a_parameter_changed_in_place():
    E, A, K, D = 5, 3, 5, 35
    actor, critic = RR.random_net(D, A, 701)
    da, dc = _dev(actor), _dev(critic)
    pol = P.RecurrentDevicePolicy(da, dc)
    obs, eps = R.random_obs(E, A, K, D, 702)
    x, e = _obs_dev(obs), _cuda(eps)
    ha, hc = (_cuda(h) for h in RR.random_states(E, A, 703))
    before = pol.forward(*x, actor_state=ha, critic_state=hc, eps=e)
    da["rnn.cell.weight_hh"].mul_(0.5)                           # a GRU weight ...
    mid = pol.forward(*x, actor_state=ha, critic_state=hc, eps=e)
    assert not torch.equal(mid.loc, before.loc) and torch.equal(mid.value, before.value)
    dc["base.linear1.weight"].mul_(0.5)                          # ... then an encoder weight
    after = pol.forward(*x, actor_state=ha, critic_state=hc, eps=e)
    assert torch.equal(after.loc, mid.loc) and not torch.equal(after.value, mid.value)
    new_a, new_c = ({k: v.cpu().numpy() for k, v in d.items()} for d in (da, dc))
    r64 = RR.forward(new_a, new_c, obs, ha.cpu().numpy(), hc.cpu().numpy(), None, eps)
    for n in RR.OUTPUTS:
        assert np.abs(getattr(after, n).cpu().double().numpy() - r64[n].numpy()).max() < 1e-4, n


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def _call(pol, x, over=None, rover=None, flags=0, packed=True, rnn_packed=True, io=True, rio=True, counter=True, shape=None):
    """hns_policy_forward_rnn with sentinel-filled outputs; `over` / `rover` replace io / rio fields.  Returns (rc, message, untouched)."""
    pol.refresh()
    xs, xo, xc, pio = pol._io(x[0].squeeze(2), x[1], x[2])
    E, A, K = xs.shape[0], xs.shape[1], xc.shape[2]
    sent = lambda *s: torch.full(s, 777.0, device="cuda")
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
    pk = pol.packed.data_ptr() + (packed if isinstance(packed, int) and not isinstance(packed, bool) else 0) if packed else None
    rk = pol.rnn_packed.data_ptr() + (rnn_packed if isinstance(rnn_packed, int) and not isinstance(rnn_packed, bool) else 0) if rnn_packed else None
    c0 = int(pol.counter)
    rc = pol._lib.hns_policy_forward_rnn(pk, rk, D, E_, A_, K_, C.byref(pio) if io else None,
                                         (C.byref(prio, rio) if isinstance(rio, int) and not isinstance(rio, bool) else C.byref(prio)) if rio else None, flags, pol.seed,
                                         pol.counter.data_ptr() if counter else None, None)
    torch.cuda.synchronize()
    untouched = all(bool((t == 777.0).all()) for t in bufs.values()) and int(pol.counter) == c0
    return rc, pol._lib.hns_last_error().decode(), untouched


VO, DET = abi.HNS_POLICY_VALUE_ONLY, abi.HNS_POLICY_DETERMINISTIC
REFUSALS = [
    # hns_policy_forward's, in its order
    ("null packed image", dict(packed=False), "packed image"),
    ("misaligned packed image", dict(packed=4), "packed image"),
    ("null io", dict(io=False), "packed image / io"),
    ("self_dim 0", dict(shape=(0, 11, 3, 5)), "self_dim"),
    ("self_dim 97", dict(shape=(97, 11, 3, 5)), "self_dim"),
    ("8 agents", dict(shape=(35, 11, 8, 5)), "num_agents"),
    ("17 cylinders", dict(shape=(35, 11, 3, 17)), "num_cylinders"),
    ("0 envs", dict(shape=(35, 0, 3, 5)), "num_envs"),
    # the recurrent call's own, behind the shape
    ("null rnn image", dict(rnn_packed=False), "GRU image"),
    ("misaligned rnn image", dict(rnn_packed=4), "GRU image"),
    ("null rio", dict(rio=False), "rnn io"),
    ("misaligned rio", dict(rio=4), "rnn io"),
    ("unknown flag", dict(flags=4), "flag"),
    ("missing obs_self", dict(over={"obs_self": None}), "observation"),
    ("missing obs_others", dict(over={"obs_others": None}), "observation"),
    ("misaligned cylinders", dict(over={"obs_cylinders": 2}), "misaligned observation"),
    ("negative stride", dict(over={"cyl_stride": (1, -1)}), "negative stride"),
    ("missing value", dict(over={"value": None}), "value"),
    ("missing action", dict(over={"action": None}), "action"),
    ("misaligned log_prob", dict(over={"log_prob": 2}), "action / log_prob"),
    ("sampling without a counter", dict(counter=False), "counter"),
    # ... and last
    ("missing critic_h_out", dict(rover={"critic_h_out": None}), "state output"),
    ("misaligned critic_h_out", dict(rover={"critic_h_out": 4}), "state output"),
    ("missing critic_h_out, value only", dict(rover={"critic_h_out": None}, flags=VO), "state output"),
    ("missing actor_h_out", dict(rover={"actor_h_out": None}), "state output"),
    ("misaligned actor_h_out", dict(rover={"actor_h_out": 8}), "state output"),
    ("misaligned actor_h_in", dict(rover={"actor_h_in": 4}), "state input"),
    ("misaligned critic_h_in", dict(rover={"critic_h_in": 4}), "state input"),
    ("misaligned critic_h_in, value only", dict(rover={"critic_h_in": 4}, flags=VO), "state input"),
]


@pytest.mark.parametrize("what, kw, word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_launch(case11, what, kw, word):
    pol, x = case11[0], case11[1]
    rc, msg, untouched = _call(pol, x, **kw)
    assert rc == abi.HNS_ERR_INVALID_ARG, what
    assert msg.startswith("hns_policy_forward_rnn: ") and word in msg, msg
    assert untouched, what


def test_refusal_order_and_what_value_only_does_not_need(case11):
    pol, x = case11[0], case11[1]
    # the first failing check names itself: the packed image before the GRU image before the flags before the states
    assert "packed image / io" in _call(pol, x, packed=False, rnn_packed=False)[1]
    assert "GRU image" in _call(pol, x, rnn_packed=False, flags=4)[1]
    assert "flag" in _call(pol, x, flags=4, rover={"critic_h_out": None})[1]
    assert "value" in _call(pol, x, over={"value": None}, rover={"critic_h_out": None})[1]
    # value only: the actor's outputs, states and the counter are not needed
    rc, msg, _ = _call(pol, x, flags=VO, over={"action": None, "log_prob": None}, rover={"actor_h_out": None, "actor_h_in": 4}, counter=False)
    assert rc == abi.HNS_OK, msg
    rc, msg, _ = _call(pol, x, flags=DET, counter=False)        # the mode draws no noise
    assert rc == abi.HNS_OK, msg
    assert pol._lib.hns_policy_rnn_pack(None, None, pol.rnn_packed.data_ptr(), None) == abi.HNS_ERR_INVALID_ARG
    n = pol._gru_net(pol.actor_rnn)
    assert pol._lib.hns_policy_rnn_pack(C.byref(n), C.byref(n), None, None) == abi.HNS_ERR_INVALID_ARG
    n.ln_b = None
    assert pol._lib.hns_policy_rnn_pack(C.byref(n), C.byref(n), pol.rnn_packed.data_ptr(), None) == abi.HNS_ERR_INVALID_ARG
    assert "GRU parameter" in pol._lib.hns_last_error().decode()


# ---- 4. the collector -----------------------------------------------------------------------------------------------------------------
N_ENVS, T_STEPS, SEQ, EPISODE = 33, 32, 16, 12


def _make_env(seed=0):
    from hns_amd.env import HideAndSeek
    cfg = config.make_cfg({"num_agents": 3, "env": {"num_envs": N_ENVS, "max_episode_length": EPISODE}}, algo={"use_TP_net": 0})
    env = HideAndSeek(cfg, headless=True)
    env.set_seed(seed)
    return env


def _net_for(env, recurrent=True):
    D = abi.self_dim(env.num_targets)
    actor, critic = RR.random_net(D, env.num_agents, 811)
    if not recurrent:
        actor, critic = ({k: v for k, v in p.items() if not k.startswith("rnn.")} for p in (actor, critic))
    return _dev(actor), _dev(critic)


def _hand_collect(env, pol, state, T, L):
    """What a user writes without the collector: copy_ stores, the states carried out of place, the flags handed over on every step, `done`
    read back on every step.  `state`: {"cur", "ha", "hc", "flags"} carried between calls."""
    buf, seg = {}, {}
    for t in range(T):
        cur = state["cur"]
        obs = cur[("agents", "observation")]
        xs, xo, xc = obs["state_self"], obs.get("state_others", None), obs["cylinders"]
        if t % L == 0:
            for k in ("ha", "hc"):
                seg.setdefault(k, []).append(state[k].clone())
        out = pol.forward(xs, xo, xc, actor_state=state["ha"], critic_state=state["hc"], is_init=state["flags"])
        pre = {"obs_self": xs, "obs_others": xo, "obs_cylinders": xc, "action": out.action, "log_probs": out.log_prob, "state_value": out.value,
               "is_init": state["flags"]}
        for k, v in pre.items():
            buf.setdefault(k, []).append(v.clone())
        state["ha"], state["hc"] = out.actor_state, out.critic_state
        nxt = env.step(env.rand_step_input(out.action))["next"]
        done = nxt["done"]
        for k, v in (("reward", nxt[("agents", "reward")]), ("done", done)):
            buf.setdefault(k, []).append(v.clone())
        if t == T - 1:
            nobs = nxt[("agents", "observation")]
            last = {"obs_self": nobs["state_self"].clone(), "obs_others": nobs["state_others"].clone(), "obs_cylinders": nobs["cylinders"].clone(),
                    "critic_rnn_state": state["hc"].clone(), "is_init": done.clone()}
        state["flags"] = done.clone()
        if bool(done.any()):
            state["cur"] = env.reset(TensorDict({"_reset": done.clone()}, env.batch_size))
        else:
            state["cur"] = nxt
    data = {k: torch.stack(v, 1) for k, v in buf.items()}
    segments = {"actor_rnn_state": torch.stack(seg["ha"], 1), "critic_rnn_state": torch.stack(seg["hc"], 1)}
    return data, segments, last


@pytest.fixture(scope="module")
def collected():
    """Two collects of the recurrent collector beside the hand loop and a non-recurrent collector on envs of one seed; clones of both
    rollouts' tensors."""
    envs = [_make_env() for _ in range(3)]
    try:
        pols = [P.RecurrentDevicePolicy(*_net_for(envs[i]), seed=5) for i in range(2)]
        col = collector.DeviceCollector(envs[0], pols[0], T_STEPS, rnn_seq_len=SEQ)
        plain = collector.DeviceCollector(envs[2], P.DevicePolicy(*_net_for(envs[2], recurrent=False), seed=5), T_STEPS)
        n = N_ENVS
        state = {"cur": envs[1].reset(), "ha": torch.zeros(n, 3, 128, device="cuda"), "hc": torch.zeros(n, 3, 128, device="cuda"),
                 "flags": torch.ones(n, 1, dtype=torch.bool, device="cuda")}
        rounds = []
        for call in range(2):
            st = col.collect()
            plain.collect()
            got = ({k: v.clone() for k, v in st.data.items()}, {k: v.clone() for k, v in st.segments.items()},
                   {k: v.clone() for k, v in st.last.items()})
            rounds.append((got, _hand_collect(envs[1], pols[1], state, T_STEPS, SEQ)))
        return {"rounds": rounds, "policy": pols[0], "launches": (st.launches, plain.storage.launches), "done_reads": (col.done_reads, plain.done_reads),
                "kwargs": set(st.recurrent_kwargs())}
    finally:
        for e in envs:
            e.close()


def test_collect_equals_the_hand_driven_loop_bit_for_bit(collected):
    for call, (got, want) in enumerate(collected["rounds"]):
        for part, g, w in zip(("data", "segments", "last"), got, want):
            assert set(g) == set(w), (call, part, set(g) ^ set(w))
            for k in w:
                assert g[k].shape == w[k].shape and g[k].dtype == w[k].dtype and torch.equal(g[k], w[k]), (call, part, k)
        data = got[0]
        steps = torch.arange(call * T_STEPS + 1, (call + 1) * T_STEPS + 1, device="cuda")
        assert torch.equal(data["done"], (steps % EPISODE == 0).view(1, -1, 1).expand(N_ENVS, -1, 1))      # boundaries inside the rollout
        first = torch.ones_like(data["is_init"][:, 0]) if call == 0 else collected["rounds"][0][0][0]["done"][:, -1]
        assert torch.equal(data["is_init"], torch.cat([first.unsqueeze(1), data["done"][:, :-1]], 1))
        assert got[1]["actor_rnn_state"].shape == (N_ENVS, T_STEPS // SEQ, 3, 128)
        assert float(got[1]["critic_rnn_state"][:, 1].abs().max()) > 0
    assert collected["kwargs"] == {"is_init", "actor_rnn_state", "critic_rnn_state", "rnn_seq_len", "last_critic_rnn_state", "last_is_init"}


def test_the_recurrent_collector_reads_and_launches_as_the_plain_one_plus_the_segment_stores(collected):
    rec, plain = collected["launches"]
    assert plain == 2 * (2 * T_STEPS + 1)
    assert rec == plain + 2 * (T_STEPS // SEQ) - 1             # one store more on a segment's first step (the very first finds the storage's zeros)
    assert collected["done_reads"][0] == collected["done_reads"][1] == (2 * T_STEPS) // EPISODE            # lock-step episodes: one read each


def test_stored_segments_rerun_from_their_stored_states_give_the_stored_values(collected):
    pol = collected["policy"]
    for call, (got, _) in enumerate(collected["rounds"]):
        data, seg, last = got
        for s in range(T_STEPS // SEQ):
            hc = seg["critic_rnn_state"][:, s].contiguous()
            for t in range(s * SEQ, (s + 1) * SEQ):
                out = pol.forward(data["obs_self"][:, t], data["obs_others"][:, t], data["obs_cylinders"][:, t], critic_state=hc,
                                  is_init=data["is_init"][:, t], value_only=True)
                assert torch.equal(out.value, data["state_value"][:, t]), (call, s, t)
                hc = out.critic_state
            nxt = seg["critic_rnn_state"][:, s + 1] if s + 1 < T_STEPS // SEQ else last["critic_rnn_state"]
            assert torch.equal(hc, nxt), (call, s)


def test_the_ops_over_a_stored_segment_agree_with_the_fused_chain(collected):
    """encode -> gru -> head over a stored 16-step segment from the stored states: the gate against the fp64 restatement of the same chain,
    for the ops and for what the fused kernel stored; the largest |log_prob_op - log_prob_fused| is the first-epoch ratio's distance from 1."""
    pol = collected["policy"]
    data, seg, _ = collected["rounds"][1][0]
    s, n = 1, 8                                                  # the second segment (non-zero start states, a boundary inside), eight envs
    ts = slice(s * SEQ, (s + 1) * SEQ)
    cpu = lambda t: t.cpu().numpy()
    actor = {**{k2: cpu(pol.actor_p[v]) for k2, v in P.ACTOR_NAMES.items() if v in pol.actor_p},
             **{"rnn." + k2: cpu(pol.actor_rnn[v]) for k2, v in rnn.NAMES.items()}}
    critic = {**{k2: cpu(pol.critic_p[v]) for k2, v in P.CRITIC_NAMES.items() if v in pol.critic_p},
              **{"rnn." + k2: cpu(pol.critic_rnn[v]) for k2, v in rnn.NAMES.items()}}
    refs = {}
    for dtype in (torch.float64, torch.float32):
        ha, hc = cpu(seg["actor_rnn_state"][:n, s]), cpu(seg["critic_rnn_state"][:n, s])
        lp, val = [], []
        for t in range(s * SEQ, (s + 1) * SEQ):
            obs = {"state_self": cpu(data["obs_self"][:n, t]), "state_others": cpu(data["obs_others"][:n, t]), "cylinders": cpu(data["obs_cylinders"][:n, t])}
            r = RR.forward(actor, critic, obs, ha, hc, cpu(data["is_init"][:n, t, 0]), None, dtype)
            scale = torch.exp(torch.as_tensor(actor["act_dist.log_std"]).to(dtype))
            a = torch.as_tensor(cpu(data["action"][:n, t])).to(dtype)
            lp.append((-((a - r["loc"]) ** 2) / (2 * scale ** 2) - torch.log(scale) - 0.5 * np.log(2 * np.pi)).sum(-1, keepdim=True).double().numpy())
            val.append(r["value"].double().numpy())
            ha, hc = r["actor_state"], r["critic_state"]
        refs[dtype] = (np.stack(lp, 1), np.stack(val, 1))
    # the ops: the segment's env-steps through an index, the features read in place as [B, A, L, 128]
    index = (torch.arange(n, device="cuda").unsqueeze(1) * T_STEPS + torch.arange(s * SEQ, (s + 1) * SEQ, device="cuda")).reshape(-1)
    obs = (data["obs_self"], data["obs_others"], data["obs_cylinders"])
    flags = data["is_init"][:n, ts, 0].reshape(n, 1, SEQ)
    with torch.no_grad():
        ys = []
        for p, gp, key in ((pol.actor_p, pol.actor_rnn, "actor_rnn_state"), (pol.critic_p, pol.critic_rnn, "critic_rnn_state")):
            enc = {k: v for k, v in p.items() if k in encoder.FIELDS}
            x = encoder.encode(enc, *obs, index).view(n, SEQ, 3, 128).transpose(1, 2)
            y, _ = rnn.gru(gp, x, seg[key][:n, s].contiguous(), flags)
            ys.append(y.transpose(1, 2))                         # [n, L, A, 128]
        loc = torch.nn.functional.linear(ys[0], pol.actor_p["head_w"], pol.actor_p["head_b"])
        scale = torch.exp(pol.actor_p["log_std"])
        lp_op = torch.distributions.Normal(loc, scale).log_prob(data["action"][:n, ts]).sum(-1, keepdim=True)
        v_op = torch.nn.functional.linear(ys[1], pol.critic_p["head_w"], pol.critic_p["head_b"])
    lp_fused, v_fused = data["log_probs"][:n, ts], data["state_value"][:n, ts]
    for tag, lp, v in (("ops", lp_op, v_op), ("fused", lp_fused, v_fused)):
        for name, h, k in (("log_prob", lp, 0), ("value", v, 1)):
            a, b = refs[torch.float64][k], refs[torch.float32][k]
            h = h.cpu().double().numpy()
            ratio = float(np.abs(h - a).max()) / max(float(np.abs(b - a).max()), 2.0 ** -24 * float(np.abs(a).max()))
            print(f"  segment {tag} {name}: ratio {ratio:.2f}")
            assert ratio <= BAR, (tag, name, ratio)
            RATIOS[f"segment-{tag}-{name}"] = ratio
    gap = float((lp_op - lp_fused).abs().max())
    print(f"  largest |log_prob_op - log_prob_fused| over the segment: {gap:.3e} (max |ratio - 1| {float((lp_op - lp_fused).exp().sub(1).abs().max()):.3e})")
    RATIOS["segment-log_prob-gap"] = gap


def test_report_ratios():
    print("recurrent policy gate ratios:", {k: (round(v, 2) if v > 1e-2 else v) for k, v in RATIOS.items()})
