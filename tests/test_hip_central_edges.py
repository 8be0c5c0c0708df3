"""The centralised critic (critic_input: state) on an MI355X past one row range of the weight-gradient kernel and at its edges:
hns_critic_train_grad_central through critic_train.value_loss_and_grad_central, hns_policy_central_forward through
CentralCriticDevicePolicy, CentralCriticDeviceLearner's cached workspace.  The cases are tests/central_cases.py's; tests/test_central_edges.py
pins their plans and conditions and shows the gate's teeth at these shapes on the CPU.

The gate is central_reference.gate_update, unchanged: e_hip <= 8 max(e_32, 2^-24 max|ref_64|) for value_loss, explained_var, grad_norm, values
and each of the 20 gradient tensors against fp64 autograd of tests/central_reference.py; each case asserts its conditions first.

Update (A, K, D; env-steps):
  past one range — (3, 5, 35; 1537) and (7, 16, 96; 1537 positions of a [40, 40] rollout through a permuted index whose positions 0, 768 and
  1 536 are -1, 2^40 and 1 600: the last tile, the whole last row range, has no live row) at tps 2, (1, 5, 20; 3073) at tps 3, which is also
  hns_critic_train_grad's bits; hns_critic_train_central_workspace_bytes equals the restated plan's total;
  half and tile fills — (7, 1, 20; 17), (2, 16, 20; 31), (6, 16, 24; 32), (3, 5, 35; 16), (3, 5, 35; 64), (3, 5, 1; 33), (1, 1, 1; 1);
  the numerical edges flat_tokens, saturated_softmax, large_obs at (3, 8, 20; 700 of 1 024 through an index);
  mixed loss regions — (3, 5, 35; 65) with huber_delta 0.7 (62 % of the env-steps hold both Huber regions, 66 % both sides of the clip) and mse;
  repeated entries — 70 draws from 40 env-steps, also bit for bit the call on the gathered tensors;
  a strided state_drones (every second row of a [S, 2 A, D + 3] tensor cut to D), flat and as [N, T, ...]: prepare_call takes the view in
  place (its last stride is 1) and the result has the contiguous call's bits;
  guard rows — the C entry on a `values` buffer 64 rows longer and on gradient tensors inside larger buffers, all sentinel-filled, with the
  workspace pre-filled with 0xFF bytes (NaN): every sentinel survives and the gradients have the package call's bits, so no unwritten slot of
  a partial row (O_EBO, O_EWO, O_HB, head rows A .. 6) reaches a gradient.
Forward (E, A, K, D): (32, 3, 5, 35), (31, 7, 1, 20), (64, 2, 16, 20), (33, 3, 5, 1), (97, 3, 5, 35) and the three numerical edges at
(64, 3, 8, 20): value within the gate, action / log_prob / loc DevicePolicy's bits; a value_only call leaves the Philox counter alone.
Learner: one CentralCriticDeviceLearner on 53 x 29 = 1 537 env-steps in one minibatch (tps 2), then on 8 x 4 in the now oversized cached
workspace: bit for bit the hand-driven sequence with a fresh workspace per call.

Measured on an MI355X (worst e_hip / max(e_32, 2^-24 max|ref_64|) per case, printed by test_report_ratios): update (3, 5, 35; 1537) 1.35,
(7, 16, 96; 1537, dead entries) 1.42, (1, 5, 20; 3073) 1.94; fills (7, 1, 20; 17) 1.25, (2, 16, 20; 31) 1.99, (6, 16, 24; 32) 1.87,
(3, 5, 35; 16) 2.25, (3, 5, 35; 64) 1.79, (3, 5, 1; 33) 2.28, (1, 1, 1; 1) 1.82; flat_tokens 1.21, saturated_softmax 0.91, large_obs 1.42;
mixed regions huber 1.38, mse 2.67; repeated entries 2.26.  Forward value: (32, 3, 5, 35) 1.02, (31, 7, 1, 20) 1.06, (64, 2, 16, 20) 1.11,
(33, 3, 5, 1) 1.25, (97, 3, 5, 35) 0.77; flat_tokens 4.94, saturated_softmax 0.12, large_obs 1.14.  The file takes 3.9 s, of which the
learner test 1.9 s and the two 1 537-step gates 0.5 and 0.4 s with their yardsticks."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import central_cases as CE
import central_learner_cases as CC
import central_reference as CR
import learner_cases as LC
import policy_reference as R
from hns_amd import abi
from hns_amd import critic_train as CT
from hns_amd import policy as P
from hns_amd import policy_train as PT

pytestmark = pytest.mark.gpu

RATIOS = {}
SENTINEL = -7.5


def _d(x):
    return torch.as_tensor(x).cuda()


def _dev(c, sd=None, **kw):
    """value_loss_and_grad_central on the device: the case's tensors in its layout (flat, or the [N, T, ...] rollout), check_index off."""
    crit = {k: _d(v) for k, v in c.critic.items()}
    lay = (lambda x: _d(x).reshape(*c.layout, *x.shape[1:])) if c.layout else _d
    out = CT.value_loss_and_grad_central(crit, lay(c.sd) if sd is None else sd, lay(c.cyl), lay(c.bv), lay(c.ret),
                                         _d(c.index) if c.index is not None else None, check_index=False, **c.kw, **kw)
    torch.cuda.synchronize()
    return crit, out


@functools.lru_cache(maxsize=None)
def _run(name):
    return _dev(CE.case(name))


def _same_bits(a, b, what):
    (c1, o1), (c2, o2) = a, b
    bad = [n for n in ("value_loss", "explained_var", "grad_norm") if not LC.bits_equal(getattr(o1, n), getattr(o2, n))]
    bad += [k for k, k2 in zip(c1, c2) if not LC.bits_equal(c1[k].grad, c2[k2].grad)]
    assert not bad, f"{what}: {bad}"


# ---------------------------------------------------------------------------------------------------------------- update
@pytest.mark.parametrize("name", CE.UPDATE_CASES)
def test_update_passes_the_fp64_gate(name):
    c = CE.case(name)
    r64, r32 = (CE.copy_refs(r) for r in CE.references(name))
    CE.check_conditions(name, r64, r32)
    A, K, D, B = c.sd.shape[1], c.cyl.shape[1], c.sd.shape[2], CE.steps(c)
    if name in CE.PAST_RANGE:
        key = (A, K, D, B)
        assert CE.central_plan(B) == CE.PLANS[key] and CE.PLANS[key][1] >= 2
        assert abi.load_library().hns_critic_train_central_workspace_bytes(B, D, A, K) == CE.central_workspace_bytes(B, D, A, K)
    if name.startswith("mixed"):
        lin, cut, gap_delta, gap_clip = CE.mixed_shares(r64, c)
        assert lin > 0.25 and cut > 0.25 and gap_delta > 1e-5 and gap_clip > 1e-5
    crit, out = _run(name)
    assert out.values.shape == (B, A, 1)
    pos = CE.live_positions(c)
    got = {"value_loss": float(out.value_loss), "explained_var": float(out.explained_var), "grad_norm": float(out.grad_norm),
           "values": out.values.cpu().numpy()[pos], "grads": {k: t.grad.cpu().double().numpy() for k, t in crit.items()}}
    if B * A == 1:                                              # the variance of one return: NaN on every side
        assert np.isnan(got["explained_var"]) and np.isnan(r64["explained_var"]) and np.isnan(r32["explained_var"])
        got["explained_var"] = r64["explained_var"] = r32["explained_var"] = 0.0
    RATIOS[name] = CR.gate_update(name, got, r64, r32)
    assert bool((crit["base.attn.in_proj_bias"].grad[128:256] == 0).all())          # in_proj_b's k third: the softmax cancels it


def test_one_agent_at_tps_3_is_the_obs_critics_update_bit_for_bit():
    """(1, 5, 20; 3073): hns_critic_train_grad on the same tensors — state_drones as obs_self, the cylinders as its [S, 1, K, 5]."""
    name = "a1k5d20s3073"
    c = CE.case(name)
    assert CE.central_plan(3073)[1] == 3
    crit, out = _run(name)
    o = {k.replace("state_drones", "state_self"): _d(v) for k, v in c.critic.items()}
    ref = CT.value_loss_and_grad(o, _d(c.sd), None, _d(c.cyl[:, None]), _d(c.bv), _d(c.ret))
    for n in ("value_loss", "explained_var", "grad_norm", "values"):
        assert torch.equal(getattr(out, n), getattr(ref, n)), n
    for k, v in crit.items():
        assert torch.equal(v.grad, o[k.replace("state_drones", "state_self")].grad), k


def test_repeated_entries_equal_the_gathered_call_bit_for_bit():
    name = "repeated"
    c = CE.case(name)
    i = c.index
    gathered = _dev(c._replace(sd=c.sd[i], cyl=c.cyl[i], bv=c.bv[i], ret=c.ret[i], index=None))
    _same_bits(_run(name), gathered, "the index against the gathered, contiguous tensors")
    assert torch.equal(_run(name)[1].values, gathered[1].values)


@pytest.mark.parametrize("layout", [None, (8, 8)], ids=["flat", "N-T"])
def test_a_strided_state_drones_is_read_in_place_with_the_same_bits(layout):
    """Every second row of a [S, 2 A, D + 3] tensor, the last axis cut to D: the view's last stride is 1, so prepare_call hands the kernel the
    view's own strides (no copy; a refusal would be the other possible contract) and the bits are the contiguous call's."""
    c = CE.case("a3k5d35s64")._replace(layout=layout)
    S, A, D = c.sd.shape
    tall = torch.full((S, 2 * A, D + 3), 9.0, device="cuda")
    tall[:, ::2, :D] = _d(c.sd)
    if layout:
        tall = tall.reshape(*layout, 2 * A, D + 3)
    view = tall[..., ::2, :D]
    assert not view.is_contiguous() and view.stride(-1) == 1 and view.stride(-2) == 2 * (D + 3)
    want = _dev(c)
    got = _dev(c, sd=view)
    _same_bits(got, want, "strided state_drones")
    assert torch.equal(got[1].values, want[1].values)
    _same_bits(want, _run("a3k5d35s64"), "the [N, T] layout against the flat one")


@pytest.mark.parametrize("shape", [(7, 16, 96, 33), (2, 1, 20, 5)], ids=["a7k16d96s33", "a2k1d20s5"])
def test_guard_rows_and_unwritten_partial_slots(shape):
    """hns_critic_train_grad_central called directly: `values` 64 rows longer than the batch, each gradient tensor inside a buffer 64 floats
    longer at either end, all pre-filled with a sentinel; the workspace pre-filled with 0xFF bytes (every float a NaN), so a partial-row slot
    that no tile writes — O_EBO, O_EWO, O_HB, head rows A .. 6, head_b's slots A .. 7 — would poison the gradient it reached."""
    A, K, D, S = shape
    c = CE._plain(A, K, D, S, shift=0.3)
    want_c, want = _dev(c)
    G = 64
    crit = {k: _d(v) for k, v in c.critic.items()}
    p = CT.central_critic_parameters(crit)
    bufs = {}
    for f, t in p.items():
        bufs[f] = torch.full((t.numel() + 2 * G,), SENTINEL, device="cuda")
        t.grad = bufs[f][G:G + t.numel()].view(t.shape)
    sd, sc = CT._central_state(_d(c.sd), _d(c.cyl))
    bv, ret = _d(c.bv), _d(c.ret)
    shp = CT._validate_central(p, sd, sc, bv, ret, None, False)
    lib = abi.load_library()
    nbytes = lib.hns_critic_train_central_workspace_bytes(S, D, A, K)
    assert nbytes == CE.central_workspace_bytes(S, D, A, K)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    net, grd, b, ws, nbytes, scal, B, st = PT.prepare_call("critic", p, sd, None, sc.unsqueeze(2), None, shp, lambda *a: nbytes, ws, None, 3,
                                                           abi.HnsCriticBatch)
    b.b_values, b.b_returns = bv.data_ptr(), ret.data_ptr()
    values = torch.full((S + G, A, 1), SENTINEL, device="cuda")
    rc = lib.hns_critic_train_grad_central(C.byref(net), C.byref(b), D, A, K, 0.1, abi.HNS_CRITIC_LOSS_HUBER, 10.0, C.byref(grd), scal[0:].data_ptr(),
                                           scal[1:].data_ptr(), scal[2:].data_ptr(), values.data_ptr(), ws.data_ptr(), nbytes, st)
    assert rc == abi.HNS_OK, lib.hns_last_error()
    torch.cuda.synchronize()
    assert bool((values[S:] == SENTINEL).all()) and torch.equal(values[:S], want.values)
    for (f, t), k in zip(p.items(), want_c):
        n = t.numel()
        assert bool((bufs[f][:G] == SENTINEL).all()) and bool((bufs[f][G + n:] == SENTINEL).all()), f
        assert LC.bits_equal(t.grad, want_c[k].grad), f
    for i, n in enumerate(("value_loss", "explained_var", "grad_norm")):
        assert LC.bits_equal(scal[i], getattr(want, n)), n


# ---------------------------------------------------------------------------------------------------------------- forward
FORWARD_SHAPES = [(32, 3, 5, 35), (31, 7, 1, 20), (64, 2, 16, 20), (33, 3, 5, 1), (97, 3, 5, 35)]
EDGE_SHAPE = (64, 3, 8, 20)


def _forward_case(shape, mode=None):
    """test_hip_policy_central._case's construction; `mode`: the critic and the state of the numerical edge (central_cases.critic's knobs)."""
    E, A, K, D = shape
    seed, net = {None: (50 + A, {}), "flat_tokens": (21, dict(embed_scale=1e-4, flat_bias=True)), "saturated_softmax": (22, dict(weight_scale=40.0)),
                 "large_obs": (23, {})}[mode]
    actor, obs_critic = R.random_net(D, A, 40 + A, log_std=R.LOG_STD)
    critic = CE.critic(D, A, seed, **net)
    obs, eps = R.random_obs(E, A, K, D, 60)
    sd, cyl = CR.random_state(E, A, K, D, 70)
    if mode == "large_obs":
        sd, cyl = (sd * np.float32(300.0)).astype(np.float32), (cyl * np.float32(300.0)).astype(np.float32)
    xs, xo, xc = _d(obs["state_self"]), (_d(obs["state_others"]) if A > 1 else None), _d(obs["cylinders"])
    return actor, obs_critic, critic, (xs, xo, xc), _d(eps), sd, cyl


def _cuda(d):
    return {k: _d(v) for k, v in d.items()}


@pytest.mark.parametrize("shape, mode", [(s, None) for s in FORWARD_SHAPES] + [(EDGE_SHAPE, m) for m in CE.EDGES],
                         ids=["e%da%dk%dd%d" % s for s in FORWARD_SHAPES] + CE.EDGES)
def test_forward_value_passes_the_fp64_gate_and_the_actor_keeps_its_bits(shape, mode):
    E, A, K, D = shape
    actor, obs_critic, critic, obs, eps, sd, cyl = _forward_case(shape, mode)
    v64, v32 = CR.value_np(critic, sd, cyl, torch.float64), CR.value_np(critic, sd, cyl, torch.float32)
    assert np.isfinite(v64).all() and np.isfinite(v32).all() and v64.any()
    pol = P.CentralCriticDevicePolicy(_cuda(actor), _cuda(critic), seed=77)
    ref = P.DevicePolicy(_cuda(actor), _cuda(obs_critic), seed=77)
    out = pol.forward(*obs, _d(sd), _d(cyl), eps=eps)
    want = ref.forward(*obs, eps=eps)
    assert out.value.shape == (E, A, 1)
    x = CR.ratio(out.value.cpu().numpy(), v64, v32)
    RATIOS[f"forward-{mode or 'e%da%dk%dd%d' % shape}"] = x
    print(f"  central value {shape} {mode}: ratio {x:.2f}")
    assert x <= CR.BAR, f"value: ratio {x:.2f}"
    for n in ("action", "log_prob", "loc"):
        assert torch.equal(getattr(out, n), getattr(want, n)), f"{n} (eps)"
    a, b = pol.forward(*obs, _d(sd), _d(cyl)), ref.forward(*obs)
    for n in ("action", "log_prob", "loc"):
        assert torch.equal(getattr(a, n), getattr(b, n)), f"{n} (seed, counter)"
    assert int(pol.counter) == int(ref.counter) == 1 and torch.equal(a.value, out.value)


def test_a_value_only_call_leaves_the_philox_counter_alone():
    actor, _, critic, obs, eps, sd, cyl = _forward_case((33, 3, 5, 35))
    sd, cyl = _d(sd), _d(cyl)
    pol = P.CentralCriticDevicePolicy(_cuda(actor), _cuda(critic), seed=9)
    plain = P.CentralCriticDevicePolicy(_cuda(actor), _cuda(critic), seed=9)
    first, first_plain = pol.forward(*obs, sd, cyl), plain.forward(*obs, sd, cyl)
    assert int(pol.counter) == 1 and torch.equal(first.action, first_plain.action)
    v = pol.forward(*obs, sd, cyl, value_only=True).value
    assert int(pol.counter) == 1 and torch.equal(v, first.value)
    second, second_plain = pol.forward(*obs, sd, cyl), plain.forward(*obs, sd, cyl)
    assert int(pol.counter) == int(plain.counter) == 2
    for n in ("action", "log_prob", "loc", "value"):
        assert torch.equal(getattr(second, n), getattr(second_plain, n)), n
    assert not torch.equal(second.action, first.action)


# ---------------------------------------------------------------------------------------------------------------- learner
def test_train_rollout_through_the_cached_workspace_is_the_hand_driven_sequence_bit_for_bit():
    """53 envs x 29 steps = 1 537 env-steps in ONE minibatch (tps 2, the last row range one tile with one live row), one epoch, predictor off;
    then 8 x 4 = 32 env-steps in the workspace the first call cached."""
    A, D, K = 3, 20, 5
    cfg = {**CC.CFG, "num_minibatches": 1, "ppo_epochs": 1}
    assert CE.central_plan(53 * 29)[:3] == (49, 2, 25) and CE.central_plan(8 * 4)[:3] == (1, 1, 1)
    state = CC.make_state(A, D, 81, "cuda")
    a, b = CC.clone_state(state), CC.clone_state(state)
    L = CC.make_learner(a, cfg, seed=5)
    opts, gen = CC.hand_optimisers(b, cfg), torch.Generator(device="cuda").manual_seed(5)
    nbytes = None
    for (N, T), seed in (((53, 29), 82), ((8, 4), 83)):
        ro = LC.to_device(CC.make_rollout(state, N, T, A, D, K, seed), "cuda")
        got = L.train_rollout(**ro)
        want = CC.hand_train_op(b, opts, ro, gen, cfg)
        torch.cuda.synchronize()
        for k, v in want.items():
            assert np.float32(got[f"drone/{k}"]) == np.float32(v), ((N, T), k, got[f"drone/{k}"], v)
        LC.assert_same_state(CC.state_tensors(a, CC.learner_opts(L)), CC.state_tensors(b, opts), f"train_rollout of {N} x {T} against the hand sequence")
        if nbytes is None:
            nbytes = L._ws["critic"].numel()
            assert nbytes == CE.central_workspace_bytes(1537, D, A, K)
    assert L._ws["critic"].numel() == nbytes > CE.central_workspace_bytes(32, D, A, K)            # the second rollout ran in the first's workspace
    assert sum(not torch.equal(a["critic"][k], state["critic"][k]) for k in a["critic"]) >= 18      # the steps moved (nearly) every critic tensor


def test_report_ratios():
    print("central edge gate ratios:", {k: round(v, 2) for k, v in RATIOS.items()})
