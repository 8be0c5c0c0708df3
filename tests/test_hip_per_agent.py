"""One actor per agent (share_actor: False) on an MI355X: hns_policy_forward_agents / hns_policy_act_agents through
hns_amd.policy.PerAgentDevicePolicy, hns_actor_train_grad_agents through hns_amd.actor_train's *_per_agent functions,
learner.PerAgentDeviceLearner, and the collector and evaluator with the per-agent policy.

Forward: for every agent a the rows (., a) are bit for bit the shared DevicePolicy's built from slice a, on the same observations, seed and
counter — the agents' parameters differ, so a tile that read another agent's image, or a row with another Philox counter, shows.

Update: the accuracy gate of test_hip_actor_train.py under its rule and its BAR = 8: for policy_loss, entropy, ESS, the gradient norm, log_probs
and EACH agent's slice of EACH gradient tensor, e_hip <= 8 max(e_32, 2^-24 max|ref_64|), errors as max-abs against fp64 autograd of
tests/actor_per_agent_reference.py, e_32 the error of the same statements in CPU torch fp32 autograd; every case asserts first, in fp64, that no
ratio is within 1e-3 of 1 +- clip_param.  No row is left out.  log_probs are bit for bit the shared path's with slice a.

Measured on an MI355X (worst e_hip / max(e_32, 2^-24 max|ref_64|) over the four scalars, log_probs and every agent's slice of every
gradient tensor; printed by test_report_ratios): (A, K, D; S, B) = (3, 5, 35; 24, 17) 1.52, (3, 5, 35; 40, 33) 2.68, (1, 5, 20; 24, 17) 0.87,
(7, 16, 24; 24, 5) 5.85, (2, 8, 20; 3, 1) 1.48; unsorted index with entropy_coef 0 3.60, all-inside 1.97, all-outside 2.40; the cross-check
against the shared path per agent 1.12 / 1.21 / 1.27; the recorded cases of g_actor_per_agent.npz: a3k5d35 1.77, a2k8d20 3.33."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import actor_per_agent_reference as UA
import actor_update_reference as U
import learner_cases as LC
import per_agent_cases as PC
from hns_amd import actor_train as AT
from hns_amd import collector, config, evaluator
from hns_amd import policy as P

pytestmark = pytest.mark.gpu

BAR = 8.0
RATIOS = {}
FORWARD_SHAPES = [(3, 5, 35, 33), (1, 5, 20, 32), (7, 16, 24, 31), (2, 8, 20, 1), (3, 5, 35, 65)]      # (A, K, D, E)


# ---------------------------------------------------------------------------------------------------------------- forward, act
def _nets(A, D, seed):
    """(the stacked actor and the critic under the reference's names on the device, the same on the CPU)."""
    actors, critic = P.random_parameters_per_agent(D, A, seed)
    g = torch.Generator().manual_seed(seed + 1)
    actors = {k: v + torch.randn(v.shape, generator=g) * (0.3 if k.endswith("log_std") else 0.05) for k, v in actors.items()}
    actors["act_dist.fc_mean.weight"] = actors["act_dist.fc_mean.weight"] * 30.0
    return {k: v.cuda().contiguous() for k, v in actors.items()}, {k: v.cuda() for k, v in critic.items()}


def _views(E, A, K, D, seed):
    """Observations as time slices of [E, T, A, ...] storage: strided in the env axis, as the collector's rollout hands them out."""
    g = torch.Generator().manual_seed(seed)
    T, t = 3, 1
    xs = (torch.randn(E, T, A, D, generator=g) * 0.7).cuda()[:, t]
    xo = (torch.randn(E, T, A, A - 1, 3, generator=g) * 0.5).cuda()[:, t] if A > 1 else None
    xc = (torch.randn(E, T, A, K, 5, generator=g) * 0.5).cuda()[:, t]
    assert not xs.is_contiguous() or E == 1
    return xs, xo, xc


def _shared(actors, critic, a, seed):
    return P.DevicePolicy({k: v[a] for k, v in actors.items()}, critic, seed=seed)


def _same_rows(got, want, a, what):
    for f in ("action", "log_prob", "value", "loc"):
        g, w = getattr(got, f), getattr(want, f)
        assert (g is None) == (w is None), (what, f)
        if g is not None:
            assert LC.bits_equal(g[:, a], w[:, a]), f"{what}: {f} of agent {a} differs from the shared policy's with its slice"


@pytest.mark.parametrize("A, K, D, E", FORWARD_SHAPES)
def test_forward_rows_are_the_shared_policys_with_the_agents_slice(A, K, D, E):
    """With the caller's eps, with Philox (the same seed and call counter), the mode, `act`, and value_only leaving the actor's outputs alone."""
    actors, critic = _nets(A, D, 10 * A + K)
    xs, xo, xc = _views(E, A, K, D, 3)
    pol = P.PerAgentDevicePolicy(actors, critic, cfg={"share_actor": False}, seed=77)
    assert pol.per_agent and tuple(pol.scale.shape) == (A, 4)
    eps = torch.randn(E, A, 4, generator=torch.Generator().manual_seed(4)).cuda()
    out_eps = pol.forward(xs, xo, xc, eps=eps)
    out_rng1, out_rng2 = pol.forward(xs, xo, xc), pol.forward(xs, xo, xc)                    # counters 0 and 1
    out_det = pol.forward(xs, xo, xc, deterministic=True)
    act = pol.act(xs, xo, xc)
    assert int(pol.counter) == 2 and not torch.equal(out_rng1.action, out_rng2.action)
    assert LC.bits_equal(act, out_det.action)
    val = pol.forward(xs, xo, xc, value_only=True)
    assert val.action is None and LC.bits_equal(val.value, out_eps.value)
    for a in range(A):
        sh = _shared(actors, critic, a, 77)
        assert LC.bits_equal(pol.scale[a], sh.scale)
        _same_rows(out_eps, sh.forward(xs, xo, xc, eps=eps), a, "eps")
        _same_rows(out_rng1, sh.forward(xs, xo, xc), a, "philox, counter 0")
        _same_rows(out_rng2, sh.forward(xs, xo, xc), a, "philox, counter 1")
        _same_rows(out_det, sh.forward(xs, xo, xc, deterministic=True), a, "mode")
        assert LC.bits_equal(act[:, a], sh.act(xs, xo, xc)[:, a])
    if A > 1:                                                    # the agents differ: a mixed-up agent cannot hide
        assert not torch.equal(out_det.action[:, 0], _shared(actors, critic, 1, 77).forward(xs, xo, xc, deterministic=True).action[:, 0])


def test_value_only_leaves_the_actors_outputs_untouched():
    """The C entry with HNS_POLICY_VALUE_ONLY on an io whose action / log_prob / loc point at poisoned memory."""
    import ctypes as C
    from hns_amd import abi
    A, K, D, E = 3, 5, 35, 33
    actors, critic = _nets(A, D, 5)
    pol = P.PerAgentDevicePolicy(actors, critic)
    xs, xo, xc = (t.contiguous() if t is not None else None for t in _views(E, A, K, D, 6))
    pol.refresh()
    xs, xo, xc, io = pol._io(xs, xo, xc)
    poison = [torch.full((E, A, n), 7.5, device="cuda") for n in (4, 1, 4)]
    value = torch.empty(E, A, 1, device="cuda")
    io.action, io.log_prob, io.loc, io.value = poison[0].data_ptr(), poison[1].data_ptr(), poison[2].data_ptr(), value.data_ptr()
    rc = pol._lib.hns_policy_forward_agents(pol.packed.data_ptr(), D, E, A, K, C.byref(io), abi.HNS_POLICY_VALUE_ONLY, 0, pol.counter.data_ptr(),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and all(bool((t == 7.5).all()) for t in poison) and int(pol.counter) == 0
    assert LC.bits_equal(value, pol.forward(xs, xo, xc, value_only=True).value)


# ---------------------------------------------------------------------------------------------------------------- update
def _net(D, A, seed):
    import test_hip_actor_train as TA
    return UA.stacked_actor(TA._net(D, A, seed), A, seed + 11)


def _obs(S, A, K, D, seed):
    import test_hip_actor_train as TA
    obs = TA._obs(S, A, K, D, seed)
    return obs


def _case(S, A, K, D, seed, B=None, adv_scale=1.0, bands=((0.0, 0.05), (0.15, 0.40)), sort=False):
    actors, obs = _net(D, A, seed), _obs(S, A, K, D, seed + 1)
    index = np.random.default_rng(seed + 3).permutation(S)[:B] if B else None
    if sort and index is not None:
        index = np.sort(index)
    action = UA.sample_actions(actors, obs, seed + 2)
    lpo = U.make_old_log_probs(UA.new_log_probs(actors, obs, action), seed + 4, bands)
    adv = (np.random.default_rng(seed + 5).standard_normal((S, A, 1)) * adv_scale).astype(np.float32)
    return actors, obs, action, lpo, adv, index


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda() if x is not None else None


def _dev_call(actors, obs, action, lpo, adv, index, fn=AT.policy_loss_and_grad_per_agent, **kw):
    c = {k: torch.as_tensor(v.copy()).cuda() for k, v in actors.items()}
    out = fn(c, _dev(obs["state_self"]), _dev(obs.get("state_others")), _dev(obs["cylinders"]), _dev(action), _dev(lpo), _dev(adv), _dev(index), **kw)
    torch.cuda.synchronize()
    return c, out


def _check(tag, items):
    worst, bad = 0.0, []
    for name, h, a, b in items:
        h, a, b = np.asarray(h, np.float64), np.asarray(a, np.float64), np.asarray(b, np.float64)
        assert h.shape == a.shape and np.isfinite(h).all(), name
        e_hip, e_32 = float(np.abs(h - a).max()), float(np.abs(b - a).max())
        bound = max(e_32, 2.0 ** -24 * float(np.abs(a).max()))
        ratio = e_hip / bound if bound > 0 else (0.0 if e_hip == 0 else math.inf)
        print(f"  {tag} {name}: e_hip {e_hip:.3e} e_32 {e_32:.3e} max|ref| {np.abs(a).max():.3e} ratio {ratio:.2f}")
        worst = max(worst, ratio)
        if not ratio <= BAR:
            bad.append(f"{name}: e_hip {e_hip:.3e} > {BAR} x {bound:.3e} (ratio {ratio:.2f})")
    RATIOS[tag] = round(worst, 2)
    assert not bad, f"{tag}: " + "; ".join(bad)


def gate(tag, actors, obs, action, lpo, adv, index, need_all=True, shared_bits=True, **kw):
    r64 = UA.loss_and_grad(actors, obs, action, lpo, adv, index, dtype=torch.float64, **kw)
    r32 = UA.loss_and_grad(actors, obs, action, lpo, adv, index, dtype=torch.float32, **kw)
    U.assert_off_the_clip(r64, kw.get("clip_param", 0.1), need_all=need_all)                  # first: the clip is a discontinuity
    assert np.array_equal(r64["w"], r32["w"]), f"{tag}: fp32 takes another side of the clip on some row"
    c, out = _dev_call(actors, obs, action, lpo, adv, index, **kw)
    A = r64["log_probs"].shape[1]
    items = [(n, float(getattr(out, n)), r64[n], r32[n]) for n in ("policy_loss", "entropy", "ess", "grad_norm")]
    assert set(c) == set(r64["grads"])
    for n in r64["grads"]:
        assert c[n].grad.shape == c[n].shape
        items += [(f"{n}[{a}]", c[n].grad[a].cpu().double().numpy(), r64["grads"][n][a], r32["grads"][n][a]) for a in range(A)]
    items.append(("log_probs", out.log_probs.cpu().double().numpy(), r64["log_probs"], r32["log_probs"]))
    _check(tag, items)
    if shared_bits:                                              # the same row-local arithmetic: the shared path's bits with slice a
        for a in range(A):
            _, sh = _dev_call(UA.agent(actors, a), obs, action, lpo, adv, index, fn=AT.policy_loss_and_grad, **kw)
            assert LC.bits_equal(out.log_probs[:, a], sh.log_probs[:, a]), f"{tag}: log_probs of agent {a}"
    return r64, c, out


@pytest.mark.parametrize("A, K, D, S, B", [(3, 5, 35, 24, 17), (3, 5, 35, 40, 33), (1, 5, 20, 24, 17), (7, 16, 24, 24, 5), (2, 8, 20, 3, 1)])
def test_update_passes_the_fp64_gate(A, K, D, S, B):
    """17 positions per agent: one partial tile each; 33: a full tile and a one-row tile; 5 positions of 7 agents; a single env-step (no row
    of some kind of the clip may occur among so few: said so)."""
    actors, obs, action, lpo, adv, index = _case(S, A, K, D, 500 + A + S, B=B)
    gate(f"a{A}k{K}d{D}-s{S}b{B}", actors, obs, action, lpo, adv, index, need_all=B * A >= 15)


def test_all_inside_all_outside_entropy_coef_0_and_an_unsorted_index():
    actors, obs, action, lpo, adv, index = _case(40, 3, 5, 35, 601, B=33)
    assert (np.diff(index) < 0).any()                            # the index is a shuffled subset: unsorted
    gate("unsorted-entropy-0", actors, obs, action, lpo, adv, index, entropy_coef=0.0)
    _, first = _dev_call(actors, obs, action, lpo, adv, index)
    own = np.zeros_like(lpo)
    own[index] = first.log_probs.cpu().numpy()
    r, _, out = gate("all-inside", actors, obs, action, own, adv, index, need_all=False)
    assert (r["w"] == 1).all() and abs(float(out.ess) - 1.0) <= 2.0 ** -22
    actors, obs, action, lpo, adv, index = _case(40, 3, 5, 35, 602, B=33, bands=((0.15, 0.40),))
    r, _, _ = gate("all-outside", actors, obs, action, lpo, adv, index, need_all=False)
    assert ((r["ratio"] < 0.9) | (r["ratio"] > 1.1)).all()


def test_cross_check_against_the_shared_path_one_agent_at_a_time():
    """entropy_coef 0 and the advantages zeroed outside agent a: the loss is agent a's rows' alone, and agent a's gradient slice is then the
    shared path's gradient with slice a on the same data (the sums differ only in order) — held to the gate with the shared path's fp64 as
    the reference; the other agents' slices are exactly zero."""
    actors, obs, action, lpo, adv, index = _case(40, 3, 5, 35, 611, B=33)
    for a in range(3):
        adv_a = np.zeros_like(adv)
        adv_a[:, a] = adv[:, a]
        c, _ = _dev_call(actors, obs, action, lpo, adv_a, index, entropy_coef=0.0)
        sl = UA.agent(actors, a)
        r64 = U.loss_and_grad(sl, obs, action, lpo, adv_a, index, entropy_coef=0.0)
        cs, _ = _dev_call(sl, obs, action, lpo, adv_a, index, fn=AT.policy_loss_and_grad, entropy_coef=0.0)
        _check(f"cross-{a}", [(n, c[n].grad[a].cpu().double().numpy(), r64["grads"][n], cs[n].grad.cpu().double().numpy()) for n in r64["grads"]])
        for n in c:
            for b in range(3):
                if b != a:
                    assert not c[n].grad[b].any(), (n, a, b)


def test_advantages_times_40_through_update_actor_per_agent_and_the_refresh_after_a_step():
    """The clip of the norm is active; the step moves the version counters, and PerAgentDevicePolicy re-packs: its next forward is the shared
    policy's on the UPDATED slices."""
    actors, obs, action, lpo, adv, index = _case(24, 3, 5, 35, 621, B=17, adv_scale=40.0)
    r64 = UA.loss_and_grad(actors, obs, action, lpo, adv, index)
    assert r64["grad_norm"] > 10.0
    c = {k: torch.nn.Parameter(torch.as_tensor(v.copy()).cuda()) for k, v in actors.items()}
    _, critic = _nets(3, 35, 1)
    pol = P.PerAgentDevicePolicy(c, critic)
    xs, xo, xc = _dev(obs["state_self"][:, :, 0]), _dev(obs["state_others"]), _dev(obs["cylinders"])
    before = pol.forward(xs, xo, xc, deterministic=True).action.clone()
    opt = AT.make_optimizer_per_agent(c, {"share_actor": False})
    st = AT.update_actor_per_agent(c, xs, xo, xc, _dev(action), _dev(lpo), _dev(adv), opt, index=_dev(index), cfg={"share_actor": False})
    assert abs(float(st["actor_grad_norm"]) - r64["grad_norm"]) <= 1e-4 * r64["grad_norm"]
    clipped = math.sqrt(sum(float((v.grad.double() ** 2).sum()) for v in c.values()))
    assert abs(clipped - 10.0) <= 1e-4 * 10.0                    # clip_grad_norm_ over the stacked tensors: one norm over all agents
    after = pol.forward(xs, xo, xc, deterministic=True).action
    assert not torch.equal(before, after)
    for a in range(3):
        sh = P.DevicePolicy({k: v.detach()[a] for k, v in c.items()}, critic)
        assert LC.bits_equal(after[:, a], sh.forward(xs, xo, xc, deterministic=True).action[:, a])


@pytest.mark.parametrize("tag", ["a3k5d35", "a2k8d20"])
def test_two_updates_against_the_reference_fixture(tag):
    """g_actor_per_agent.npz (the reference's update_actor with share_actor: False, recorded): the gate on update 1, the scalars of both updates
    and the parameters after two updates at test_hip_actor_train.py's tolerances for g_actor_update.npz (1e-5 relative on policy_loss, entropy
    and ESS of update 1, 1e-4 on the gradient norm) — a wrong loss scale or entropy share fails here."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    actors, obs, action, lpo, adv, index, ent_coef, rec = UA.golden_case(np.load(os.path.join(here, "g_actor_per_agent.npz")),
                                                                         np.load(os.path.join(here, "g_policy.npz")), tag)
    _, _, out = gate(f"golden-{tag}", actors, obs, action, lpo, adv, index, entropy_coef=ent_coef)
    assert abs(float(out.policy_loss) - float(rec["u1:policy_loss"])) <= 1e-5 * abs(float(rec["u1:policy_loss"]))
    assert abs(float(out.entropy) - float(rec["u1:entropy"])) <= 1e-5 * float(rec["u1:entropy"])
    assert abs(float(out.ess) - float(rec["u1:ESS"])) <= 1e-5 * float(rec["u1:ESS"])
    assert abs(float(out.grad_norm) - float(rec["u1:grad_norm"])) <= 1e-4 * float(rec["u1:grad_norm"])
    c = {k: torch.nn.Parameter(torch.as_tensor(v.copy()).cuda()) for k, v in actors.items()}
    cfg = {"share_actor": False, "clip_param": 0.1, "entropy_coef": ent_coef, "max_grad_norm": 10.0, "actor": {"lr": 5e-4}}
    opt = AT.make_optimizer_per_agent(c, cfg)
    for u in (1, 2):
        st = AT.update_actor_per_agent(c, _dev(obs["state_self"]), _dev(obs["state_others"]), _dev(obs["cylinders"]), _dev(action), _dev(lpo), _dev(adv),
                                       opt, index=_dev(index), cfg=cfg)
        if u == 1:
            assert abs(float(st["actor_grad_norm"]) - float(rec["u1:grad_norm"])) <= 1e-4 * float(rec["u1:grad_norm"])
    # Adam's step is lr x (a number of magnitude <= 1 early on): after two steps a parameter is within 2 lr of its start whatever the gradient's
    # last bits; where the recorded and the device gradients agree in sign and to fp32 error the results agree far closer: 1e-5 absolute, the
    # bound the shared fixture test's end-to-end comparison uses for two steps at lr 5e-4 (2 % of one step)
    for k, v in c.items():
        if f"final:{k}" in rec and "in_proj_bias" not in k:
            assert np.abs(v.detach().cpu().numpy() - rec[f"final:{k}"]).max() <= 1e-5, k


def test_the_same_call_twice_gives_the_same_bits():
    actors, obs, action, lpo, adv, index = _case(40, 3, 5, 35, 631, B=33)
    c1, o1 = _dev_call(actors, obs, action, lpo, adv, index)
    c2, o2 = _dev_call(actors, obs, action, lpo, adv, index)
    assert all(LC.bits_equal(getattr(o1, f), getattr(o2, f)) for f in o1._fields)
    assert all(LC.bits_equal(c1[k].grad, c2[k].grad) for k in c1)


# ---------------------------------------------------------------------------------------------------------------- learner
@pytest.mark.parametrize("use_tp", [False, True])
def test_train_rollout_is_the_hand_driven_sequence_bit_for_bit(use_tp):
    """8 envs x 8 steps x 3 agents, 2 epochs x 2 minibatches, predictor off and on; and the device's info row against the CPU path's."""
    N, T, A = 8, 8, 3
    cpu = PC.make_state(A, 41)
    ro_cpu = PC.make_rollout(cpu, N, T, A, 42)
    ro = LC.to_device(ro_cpu, "cuda")
    kw = lambda r: {k: v for k, v in r.items() if k != "tp"} | ({"tp": r["tp"]} if use_tp else {})      # noqa: E731
    hand_state = PC.clone_state(cpu, "cuda")
    opts = PC.hand_optimisers(hand_state)
    hand = PC.hand_train_op(hand_state, opts, ro, torch.Generator(device="cuda").manual_seed(5), use_tp=use_tp)
    state = PC.clone_state(cpu, "cuda")
    L = PC.make_learner(state, seed=5, use_tp=use_tp)
    info = L.train_rollout(**kw(ro))
    torch.cuda.synchronize()
    if not use_tp:
        opts["tp"] = None
    LC.assert_same_state(LC.state_tensors(state, LC.learner_opts(L)), LC.state_tensors(hand_state, opts), "device train_rollout against the hand sequence")
    PC.check_info(info, hand, use_tp)
    assert set(L._ws) == {"actor", "critic", "info"}


def test_the_device_agrees_with_the_cpu_path_on_the_info_row(monkeypatch):
    """One train_rollout on each device with every permutation drawn from ONE CPU generator (test_hip_learner.py's run_with_fixed_rows: the two
    devices' generators differ), predictor on.  Every scalar of the row is a mean over the 4 updates of numbers the update gate holds to fp32's
    error at equal parameters; after a step the two sides' parameters differ by Adam steps on gradients that differ at fp32's error, which is
    second order for the scalars.  Bound: 1e-4 relative (floor 1e-4), two decades above fp32's error over 96-row means and two below a change
    that matters (a wrong entropy share moves `entropy`'s gradient, hence the row, by percents over the steps); the figures are printed.
    Measured on an MI355X: the largest difference 9.5e-7 (actor_grad_norm 9.326), the others at most 4.8e-7, seven of twelve entries equal."""
    from hns_amd import learner
    N, T, A = 8, 8, 3
    cpu = PC.make_state(A, 41)
    ro = PC.make_rollout(cpu, N, T, A, 42)
    infos = {}
    for device in ("cpu", "cuda"):
        gen = torch.Generator().manual_seed(7)
        monkeypatch.setattr(learner.tp_train, "minibatches", lambda n, m, dev, generator=None: torch.randperm((n // m) * m, generator=gen).reshape(m, -1).to(dev))
        infos[device] = PC.make_learner(PC.clone_state(cpu, device), seed=0).train_rollout(**LC.to_device(ro, device))
    assert set(infos["cpu"]) == set(infos["cuda"])
    bad = []
    for k, c in infos["cpu"].items():
        d = infos["cuda"][k]
        print(f"  {k}: cpu {c:.7g} device {d:.7g} |diff| {abs(d - c):.2e}")
        if not abs(d - c) <= 1e-4 * max(1.0, abs(c)):
            bad.append(k)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- collector, evaluator
TASK = {"num_agents": 3, "env": {"num_envs": 33, "max_episode_length": 5}}


def _env_policy(env, seed):
    from hns_amd import abi
    D = abi.self_dim(env.num_targets)
    actors, critic = P.random_parameters_per_agent(D, env.num_agents, seed)
    actors["act_dist.fc_mean.weight"] = actors["act_dist.fc_mean.weight"] * 30.0    # actions of order 0.3: the drones move
    g = torch.Generator().manual_seed(seed + 1)
    actors["act_dist.log_std"] = actors["act_dist.log_std"] + torch.randn(actors["act_dist.log_std"].shape, generator=g) * 0.3
    return P.PerAgentDevicePolicy(actors, critic, device=env.device, seed=seed)


def test_collect_with_the_per_agent_policy_equals_the_hand_driven_loop():
    """4 steps of DeviceCollector.collect at 33 envs, twice, against test_hip_collector.py's hand loop (env.step + policy.forward + copies)
    with a per-agent policy of the same seed: every learner tensor bit for bit.  The collector needed no change."""
    import test_hip_collector as TC
    task = {"num_agents": 3, "env": {"num_envs": 33}}
    envs = [TC._make_env(task, 0, 0) for _ in range(2)]
    try:
        col, hand = collector.DeviceCollector(envs[0], _env_policy(envs[0], 9), 4), TC.HandLoop(envs[1], _env_policy(envs[1], 9), 4)
        for call in range(2):
            TC._same_kwargs(col.collect().learner_kwargs(), hand.collect(), f"collect {call}")
    finally:
        for e in envs:
            e.close()


def test_evaluate_with_the_per_agent_policy_equals_the_hand_driven_loop():
    """A 5-step evaluate() at 33 envs against test_hip_evaluator.py's hand loop with the per-agent policy's deterministic forward: the
    statistics bit for bit (evaluate runs `act`, the hand loop `forward(deterministic=True)`).  The evaluator needed no change."""
    import test_hip_evaluator as TE
    from hns_amd import abi
    L = 5
    env, hand = TE._make_env(TASK, 0), TE._make_env(TASK, 0)
    try:
        pol = _env_policy(env, 8)
        ev = evaluator.DeviceEvaluator(env, pol)
        info = ev.evaluate(seed=3)
        assert ev.steps == L
        hand.set_seed(3)
        cur = hand.reset()
        for _ in range(L):
            obs = cur[("agents", "observation")]
            out = pol.forward(obs["state_self"], obs.get("state_others", None), obs["cylinders"], deterministic=True)
            cur = hand.step(hand.rand_step_input(out.action))["next"]
        assert bool(cur["done"].all())
        for k in abi.STAT_NAMES:
            assert LC.bits_equal(ev.stats[k], hand.stats[k].reshape(-1)), k
        assert set(info) == {"eval/stats." + k for k in abi.STAT_NAMES}
    finally:
        env.close()
        hand.close()


def test_report_ratios():
    print("worst e_hip / max(e_32, 2^-24 max|ref_64|) per case:", RATIOS)
