"""The actor's update on the device (hns_actor_train_grad, hns_adam_clipped through hns_amd.actor_train) on an MI355X.

Accuracy gate (the rule of test_hip_critic_train.py, BAR = 8): for policy_loss, entropy, ESS, the gradient norm, log_probs and EACH of the
actor's gradient tensors, e_hip <= 8 max(e_32, 2^-24 max|ref_64|), errors as max-abs against fp64 autograd of
tests/actor_update_reference.py, e_32 the error of the same statements in CPU torch fp32 autograd.  The clip of the ratio is a discontinuity:
every case builds log_probs_old = logp_new - delta with |delta| in [0, 0.05] or [0.15, 0.40] and asserts first, in fp64 on the CPU, that no
ratio is within 1e-3 of 1 +- clip_param and that rows with w = 0, rows with w = 1 outside the clip and rows inside it all occur (except in the
all-inside and all-outside cases and the 3-row minibatch of test_shape_limits, which say so).  No row is left out of any comparison.  Worst ratio per case: printed by test_report_ratios.

Measured on an MI355X (worst e_hip / max(e_32, 2^-24 max|ref_64|) over the four scalars, log_probs and the gradient tensors):
  fixture shapes (default / advantages x 40 / entropy_coef 0 / log_std per component): a3k5d35 0.89 / 1.08 / 0.89 / 1.15, a3k8d20 1.51 / 1.18 /
  1.51 / 1.40, a1k5d20 1.78 / 2.83 / 1.78 / 1.31, a6k16d24 1.44 / 1.17 / 1.44 / 1.03; the recorded cases of g_actor_update.npz: a3k5d35 1.05,
  a3k8d20 1.35, a1k5d20 1.51 (8.68 on d fc_mean.bias while the log-probability was summed in fp32: the kernel now forms it in fp64),
  a6k16d24 1.63; all-inside 0.97, all-outside 1.67; 8 192 of the 131 072 env-steps of a [2048, 64] rollout 3.96; a full 65 536-env-step
  minibatch 3.03; flat_tokens 3.73, saturated_softmax 1.75, large_obs 1.45, actions 8 sigma out 0.32; shape limits: A = 1 1.25, A = 7 1.46,
  K = 1 1.19, K = 16 3.59, D = 1 0.98, D = 96 1.43, one env-step 1.62, 33 rows 2.12.
  End to end (64 updates of actor and critic interleaved): actor max |device - cpu| 1.1e-3, median 3.7e-9; critic 3.1e-5, 2.3e-9."""
import math
import os

import numpy as np
import pytest
import torch

import actor_update_reference as U
import critic_update_reference as UC
import policy_reference as R
from hns_amd import actor_train as AT
from hns_amd import critic_train as CT
from hns_amd import policy as P

pytestmark = pytest.mark.gpu

BAR = 8.0
RATIOS = {}


def _net(D, A, seed, weight_scale=1.0, embed_scale=1.0, flat_bias=False, log_std=None):
    actor, _ = P.random_parameters(D, A, seed)
    g = torch.Generator().manual_seed(seed + 7)
    for k, v in actor.items():
        if (k.endswith("bias") or "norm" in k) and "fc_mean" not in k:
            actor[k] = v + torch.randn(v.shape, generator=g) * 0.1
        if "in_proj_weight" in k:
            actor[k] = actor[k] * weight_scale
        if "split_embed.embed" in k and k.endswith("weight"):
            actor[k] = actor[k] * embed_scale
        if k == "act_dist.fc_mean.weight":
            actor[k] = v * 30.0                                # means of order 0.3
        if k == "act_dist.fc_mean.bias":
            actor[k] = v + torch.randn(v.shape, generator=g) * 0.1
        if k == "act_dist.log_std" and log_std is not None:
            actor[k] = torch.tensor(log_std)
    actor = {k: v.numpy().astype(np.float32) for k, v in actor.items()}
    if flat_bias:
        for k in actor:
            if "split_embed.embed" in k and k.endswith("bias"):
                actor[k] = (np.full_like(actor[k], 0.3) + np.linspace(0, 1e-3, actor[k].size, dtype=np.float32)).astype(np.float32)
    return actor


def _obs(S, A, K, D, seed, scale=1.0):
    g = np.random.default_rng(seed)
    obs = {"state_self": (g.standard_normal((S, A, 1, D)) * 0.7 * scale).astype(np.float32)}
    if A > 1:
        obs["state_others"] = (g.standard_normal((S, A, A - 1, 3)) * 0.5 * scale).astype(np.float32)
    obs["cylinders"] = (g.standard_normal((S, A, K, 5)) * 0.5 * scale).astype(np.float32)
    return obs


def _rollout(actor, obs, seed, index=None, adv_scale=1.0, sigmas=1.0, bands=((0.0, 0.05), (0.15, 0.40)), chunk=4096):
    """Actions mu + sigma eps, log_probs_old = logp_new - delta off the clip, advantages of both signs, over the env-steps of the minibatch
    (the env-steps outside `index` are never read: zeros).  mu is the restatement's fp32 forward pass; logp_new follows from it in fp64
    (fp32's error on it, ~1e-6, is far inside the 0.039 margin of delta)."""
    S, A = obs["state_self"].shape[:2]
    need = np.sort(np.asarray(index)) if index is not None else np.arange(S)
    p = {k: torch.as_tensor(v) for k, v in actor.items()}
    mus = []
    with torch.no_grad():
        for s in range(0, len(need), chunk):
            o = {k: torch.as_tensor(v[need[s:s + chunk]]) for k, v in obs.items()}
            mus.append(R._lin(R.encoder(p, "encoder.", o, torch.float32), p["act_dist.fc_mean.weight"], p["act_dist.fc_mean.bias"]).numpy())
    mu = np.concatenate(mus).astype(np.float64)
    g = np.random.default_rng(seed)
    ls = actor["act_dist.log_std"].astype(np.float64)
    act = (mu + np.exp(ls) * g.standard_normal(mu.shape) * sigmas).astype(np.float32)
    logp = (-((act - mu) ** 2) / (2 * np.exp(2 * ls)) - ls - math.log(math.sqrt(2 * math.pi))).sum(-1, keepdims=True)
    action, lpo, adv = np.zeros((S, A, 4), np.float32), np.zeros((S, A, 1), np.float32), np.zeros((S, A, 1), np.float32)
    action[need], lpo[need] = act, U.make_old_log_probs(logp, seed + 1, bands)
    adv[need] = (g.standard_normal((len(need), A, 1)) * adv_scale).astype(np.float32)
    return action, lpo, adv


def _dev_call(actor, obs, action, lpo, adv, index, shape=None, **kw):
    """Runs policy_loss_and_grad on the device; obs as [S, A, ..] (flat) or, with shape = (N, T), as the [N, T, A, ..] rollout."""
    c = {k: torch.as_tensor(v).cuda() for k, v in actor.items()}
    def lay(x):
        t = torch.as_tensor(x).cuda()
        return t.reshape(*shape, *t.shape[1:]) if shape else t
    xs, xc = lay(obs["state_self"]), lay(obs["cylinders"])
    xo = lay(obs["state_others"]) if "state_others" in obs else None
    idx = torch.as_tensor(np.asarray(index)).cuda() if index is not None else None
    out = AT.policy_loss_and_grad(c, xs, xo, xc, lay(action), lay(lpo), lay(adv), idx, **kw)
    torch.cuda.synchronize()
    return c, out


def gate(tag, actor, obs, action, lpo, adv, index, shape=None, need_all=True, **kw):
    r64 = U.loss_and_grad(actor, obs, action, lpo, adv, index, dtype=torch.float64, **kw)
    r32 = U.loss_and_grad(actor, obs, action, lpo, adv, index, dtype=torch.float32, **kw)
    U.assert_off_the_clip(r64, kw.get("clip_param", 0.1), need_all=need_all)
    assert np.array_equal(r64["w"], r32["w"]), f"{tag}: fp32 takes another side of the clip on some row"
    c, out = _dev_call(actor, obs, action, lpo, adv, index, shape, **kw)
    worst, bad = 0.0, []
    items = [(n, float(getattr(out, n)), r64[n], r32[n]) for n in ("policy_loss", "entropy", "ess", "grad_norm")]
    assert set(c) == set(r64["grads"])
    items += [(n, c[n].grad.cpu().double().numpy(), r64["grads"][n], r32["grads"][n]) for n in r64["grads"]]
    items.append(("log_probs", out.log_probs.cpu().double().numpy(), r64["log_probs"], r32["log_probs"]))
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
    return r64, out


def _case(S, A, K, D, seed, B=None, adv_scale=1.0, obs_scale=1.0, sigmas=1.0, bands=((0.0, 0.05), (0.15, 0.40)), **net):
    actor = _net(D, A, seed, **net)
    obs = _obs(S, A, K, D, seed + 1, obs_scale)
    index = np.random.default_rng(seed + 3).permutation(S)[:B] if B else None
    action, lpo, adv = _rollout(actor, obs, seed + 2, index, adv_scale, sigmas, bands)
    return actor, obs, action, lpo, adv, index


@pytest.mark.parametrize("shape", [(3, 5, 35), (3, 8, 20), (1, 5, 20), (6, 16, 24)])
@pytest.mark.parametrize("variant", ["default", "adv_x40", "entropy_coef_0", "log_std"])
def test_fixture_shapes_pass_the_fp64_gate(shape, variant):
    """The four shapes of g_policy.npz with a strict shuffled subset of the env-steps as the index: the defaults, advantages times 40 (the
    gradient norm exceeds max_grad_norm 10), entropy_coef 0, and a log_std that differs per component."""
    A, K, D = shape
    kw = {"entropy_coef": 0.0} if variant == "entropy_coef_0" else {}
    net = {"log_std": [-0.5, 0.2, 0.6, -0.1]} if variant == "log_std" else {}
    actor, obs, action, lpo, adv, index = _case(48, A, K, D, 100 + A + K, B=37, adv_scale=40.0 if variant == "adv_x40" else 1.0, **net)
    r, _ = gate(f"a{A}k{K}d{D}-{variant}", actor, obs, action, lpo, adv, index, **kw)
    if variant == "adv_x40":
        assert r["grad_norm"] > 10.0


@pytest.mark.parametrize("tag", ["a3k5d35", "a3k8d20", "a1k5d20", "a6k16d24"])
def test_golden_fixture_cases_pass_the_fp64_gate(tag):
    """The cases of g_actor_update.npz (the reference's own update_actor, recorded): the gate against fp64, and the device's scalars within
    1e-5 (policy_loss, entropy, ESS) / 1e-4 (the gradient norm) relative of the recorded fp32 ones, as the critic's golden test words it."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    actor, obs, action, lpo, adv, index, ent_coef, rec = U.golden_case(np.load(os.path.join(here, "g_actor_update.npz")), np.load(os.path.join(here, "g_policy.npz")), tag)
    _, out = gate(f"golden-{tag}", actor, obs, action, lpo, adv, index, entropy_coef=ent_coef)
    assert abs(float(out.policy_loss) - float(rec["u1:policy_loss"])) <= 1e-5 * abs(float(rec["u1:policy_loss"]))
    assert abs(float(out.entropy) - float(rec["u1:entropy"])) <= 1e-5 * float(rec["u1:entropy"])
    assert abs(float(out.ess) - float(rec["u1:ESS"])) <= 1e-5 * float(rec["u1:ESS"])
    assert abs(float(out.grad_norm) - float(rec["u1:grad_norm"])) <= 1e-4 * float(rec["u1:grad_norm"])


def test_all_inside_and_all_outside_minibatches():
    """All inside: log_probs_old is the device's own log_probs, so every ratio is exactly 1 on the device: ESS is 1 and policy_loss is
    -4 mean(adv), both within the gate against fp64 (where the ratios are 1 +- 1e-6, far inside the clip).  All outside: |delta| >= 0.15 on
    every row."""
    actor, obs, action, lpo, adv, index = _case(64, 3, 5, 35, 301, B=50)
    _, first = _dev_call(actor, obs, action, lpo, adv, index)
    own = np.zeros_like(lpo)
    own[index] = first.log_probs.cpu().numpy()
    r, out = gate("all-inside", actor, obs, action, own, adv, index, need_all=False)
    assert (r["w"] == 1).all() and np.abs(r["ratio"] - 1).max() < 1e-4
    assert torch.equal(out.log_probs, first.log_probs)
    assert abs(float(out.ess) - 1.0) <= 2.0 ** -22
    want = -4.0 * float(adv[index].astype(np.float64).mean())
    assert abs(float(out.policy_loss) - want) <= 2.0 ** -22 * max(1.0, abs(want))
    actor, obs, action, lpo, adv, index = _case(64, 3, 5, 35, 302, B=50, bands=((0.15, 0.40),))
    r, _ = gate("all-outside", actor, obs, action, lpo, adv, index, need_all=False)
    assert ((r["ratio"] < 0.9) | (r["ratio"] > 1.1)).all() and (r["w"] == 0).any() and (r["w"] == 1).any()


def test_random_minibatch_of_a_rollout_read_in_place():
    """A rollout of 2 048 envs x 64 steps read in place, an index of 8 192 of its 131 072 env-steps (24 576 rows: the reference default
    minibatch); the fp64 yardstick gathers the minibatch first, so only it is held in fp64."""
    actor, obs, action, lpo, adv, index = _case(2048 * 64, 3, 5, 35, 411, B=8192)
    assert index.max() > 2 ** 16
    gate("random-411", actor, obs, action, lpo, adv, index, shape=(2048, 64))


def test_full_65536_env_step_minibatch_passes_the_fp64_gate():
    """65 536 env-steps (196 608 rows) without an index; the fp64 yardstick runs in chunks of 8 192 env-steps."""
    actor, obs, action, lpo, adv, index = _case(65536, 3, 5, 35, 421)
    gate("full-65536", actor, obs, action, lpo, adv, None)


@pytest.mark.parametrize("mode", ["flat_tokens", "saturated_softmax", "large_obs", "action_8_sigma"])
def test_numerical_edges_pass_the_fp64_gate(mode):
    """test_hip_policy.py's three edges, and actions 8 sigma from the mean (log-probabilities near -130: the ratio is the exponential of a
    difference of two large numbers)."""
    if mode == "flat_tokens":
        case = _case(1024, 3, 8, 20, 21, B=700, embed_scale=1e-4, flat_bias=True)
    elif mode == "saturated_softmax":
        case = _case(1024, 3, 8, 20, 22, B=700, weight_scale=40.0)
    elif mode == "large_obs":
        case = _case(1024, 3, 8, 20, 23, B=700, obs_scale=300.0)
    else:
        case = _case(1024, 3, 8, 20, 24, B=700, sigmas=8.0)
    gate(mode, *case)


@pytest.mark.parametrize("shape", [(1, 5, 20, 40), (7, 5, 20, 9), (3, 1, 20, 33), (3, 16, 20, 33), (3, 5, 1, 33), (3, 5, 96, 33), (3, 5, 35, 1), (3, 5, 35, 11)])
def test_shape_limits(shape):
    """A = 1 and 7, K = 1 and 16, self_dim 1 and 96, a minibatch of one env-step and one whose row count is not a multiple of 32.  The
    one-env-step minibatch has 3 rows: too few for all three kinds of rows (w = 0, w = 1 outside the clip, inside) to be required; every other
    case here requires them.  The distance of every ratio from the clip's bounds is asserted in all of them."""
    A, K, D, B = shape
    actor, obs, action, lpo, adv, index = _case(48, A, K, D, 500 + A + K + D + B, B=B)
    gate(f"limit-a{A}k{K}d{D}b{B}", actor, obs, action, lpo, adv, index, need_all=B * A >= 20)


def _grads(c):
    return {k: v.grad.clone() for k, v in c.items()}


def test_bit_identity_across_calls_index_layout_and_graph_replay():
    actor, obs, action, lpo, adv, index = _case(32 * 16, 3, 5, 35, 611, B=300)
    c1, o1 = _dev_call(actor, obs, action, lpo, adv, index, shape=(32, 16))
    c2, o2 = _dev_call(actor, obs, action, lpo, adv, index, shape=(32, 16))
    g1 = _grads(c1)
    for k in g1:
        assert torch.equal(g1[k], c2[k].grad), k
    for n in ("policy_loss", "entropy", "ess", "grad_norm", "log_probs"):
        assert torch.equal(getattr(o1, n), getattr(o2, n)), n
    # the index against an explicit gather, [N, T, ..] strided against flat contiguous
    gathered = {k: v[index] for k, v in obs.items()}
    c3, o3 = _dev_call(actor, gathered, action[index], lpo[index], adv[index], None)
    for k in g1:
        assert torch.equal(g1[k], c3[k].grad), k
    for n in ("policy_loss", "entropy", "ess", "grad_norm", "log_probs"):
        assert torch.equal(getattr(o1, n), getattr(o3, n)), n
    wide = {k: np.concatenate([v, np.zeros_like(v)], axis=-1) for k, v in obs.items()}       # a view with strides: the last dim cut from twice the width
    c = {k: torch.as_tensor(v).cuda() for k, v in actor.items()}
    lay = lambda x: torch.as_tensor(x).cuda().reshape(32, 16, *x.shape[1:])
    xs, xo, xc = (lay(wide[k])[..., :obs[k].shape[-1]] for k in ("state_self", "state_others", "cylinders"))
    assert not xs.is_contiguous()
    idx = torch.as_tensor(index).cuda()
    o4 = AT.policy_loss_and_grad(c, xs, xo, xc, lay(action), lay(lpo), lay(adv), idx)
    for k in g1:
        assert torch.equal(g1[k], c[k].grad), k
    assert torch.equal(o1.policy_loss, o4.policy_loss) and torch.equal(o1.ess, o4.ess)
    # eager against one replay of a single-stream capture of policy_loss_and_grad + step
    def fresh():
        cc = {k: torch.as_tensor(v).cuda() for k, v in actor.items()}
        return cc, AT.make_optimizer(cc)
    ce, oe = fresh()
    xs, xo, xc = (lay(obs[k]) for k in ("state_self", "state_others", "cylinders"))
    ad, ld, vd = lay(action), lay(lpo), lay(adv)
    for _ in range(2):
        out = AT.policy_loss_and_grad(ce, xs, xo, xc, ad, ld, vd, idx)
        oe.step(grad_norm=out.grad_norm)
    cg, og = fresh()
    out = AT.policy_loss_and_grad(cg, xs, xo, xc, ad, ld, vd, idx)        # eager first step: allocates .grad and the optimizer state
    og.step(grad_norm=out.grad_norm)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = AT.policy_loss_and_grad(cg, xs, xo, xc, ad, ld, vd, idx, check_index=False)
        og.step(grad_norm=out.grad_norm)
    graph.replay()
    torch.cuda.synchronize()
    for k in ce:
        assert torch.equal(ce[k], cg[k]), k
    assert float(next(iter(og.state.values()))["step"]) == 2.0


@pytest.mark.parametrize("max_norm", [10.0, 1e9, float("inf")])
def test_adam_clipped_on_the_actors_23_tensors_matches_the_numpy_restatement_bit_for_bit(max_norm):
    g = np.random.default_rng(9)
    shapes = [(128, 35), (128,), (128, 3), (128,), (128, 5), (128,), (128,), (128,), (384, 128), (384,), (128, 128), (128,), (128, 128), (128,),
              (128, 128), (128,), (128,), (128,), (128,), (128,), (4,), (4, 128), (4,)]
    assert len(shapes) == 23
    ps = [g.standard_normal(s).astype(np.float32) for s in shapes]
    ms, vs, step = [np.zeros(s, np.float32) for s in shapes], [np.zeros(s, np.float32) for s in shapes], np.float32(0)
    dev = [torch.nn.Parameter(torch.as_tensor(p).cuda()) for p in ps]
    opt = CT.ClippedAdam(dev, lr=5e-4, max_grad_norm=max_norm)
    for it in range(3):
        gs = [(g.standard_normal(s) * 0.1 * 10.0 ** (it - 1)).astype(np.float32) for s in shapes]
        norm = np.float32(math.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for x in gs)))
        for p, x in zip(dev, gs):
            p.grad = torch.as_tensor(x).cuda()
        opt.step(grad_norm=torch.tensor(norm, device="cuda"))
        ps, cg, ms, vs, step = UC.clip_adam_np(ps, gs, ms, vs, step, norm, max_norm)
        torch.cuda.synchronize()
        for k, (p, x) in enumerate(zip(dev, ps)):
            assert np.array_equal(p.detach().cpu().numpy(), x), (it, k)
            assert np.array_equal(p.grad.cpu().numpy(), cg[k]), (it, k)
            assert np.array_equal(opt.state[p]["exp_avg"].cpu().numpy(), ms[k]) and np.array_equal(opt.state[p]["exp_avg_sq"].cpu().numpy(), vs[k])
        assert float(opt.state[dev[0]]["step"]) == it + 1 == float(step)


def test_actor_and_critic_updates_interleaved_end_to_end_and_the_policy_follows():
    """Four epochs x 16 minibatches, update_actor then update_critic on each, from the same start and the same permutations on the device and
    in CPU torch.  The bounds are test_hip_critic_train.py's (derived in its docstring): every parameter within 64 steps x lr x 0.05 = 1.6e-3
    absolute, the median |difference| at most 64 x lr x 1e-4 = 3.2e-6, for both networks.  Afterwards DevicePolicy.forward follows the new
    parameters without an explicit refresh: loc within 1e-4 of an fp64 forward pass of them."""
    S = 16 * 32
    actor = _net(35, 3, 711)
    _, critic = P.random_parameters(35, 3, 712)
    critic = {k: v.numpy() for k, v in critic.items()}
    obs = _obs(S, 3, 5, 35, 713)
    action, lpo, adv = _rollout(actor, obs, 714)
    g = np.random.default_rng(715)
    bv, ret = g.standard_normal((S, 3, 1)).astype(np.float32) * 0.1, g.standard_normal((S, 3, 1)).astype(np.float32)
    nets = {}
    for d in ("cpu", "cuda"):
        a = {k: torch.nn.Parameter(torch.as_tensor(v).to(d)) for k, v in actor.items()}
        c = {k: torch.nn.Parameter(torch.as_tensor(v).to(d)) for k, v in critic.items()}
        nets[d] = (a, c, AT.make_optimizer(a), CT.make_optimizer(c))
    pol = P.DevicePolicy(nets["cuda"][0], nets["cuda"][1])
    t = lambda x, d: torch.as_tensor(x).to(d)
    data = {d: [t(obs["state_self"], d), t(obs["state_others"], d), t(obs["cylinders"], d)] for d in nets}
    before = pol.forward(*data["cuda"], deterministic=True).loc.clone()
    gen = torch.Generator().manual_seed(3)
    for _ in range(4):
        perm = torch.randperm(S, generator=gen).reshape(16, -1)
        for idx in perm:
            for d, (a, c, oa, oc) in nets.items():
                st = AT.update_actor(a, *data[d], t(action, d), t(lpo, d), t(adv, d), oa, index=idx.to(d))
                assert st["policy_loss"].dim() == 0 and st["ESS"].device.type == d
                CT.update_critic(c, *data[d], t(bv, d), t(ret, d), oc, index=idx.to(d))
    lr, steps = 5e-4, 64
    for which in (0, 1):
        cpu, dev = nets["cpu"][which], nets["cuda"][which]
        diffs = np.concatenate([(dev[k].detach().cpu() - cpu[k].detach()).abs().numpy().ravel() for k in cpu])
        print(f"  end to end ({'actor' if which == 0 else 'critic'}): max |dev - cpu| {diffs.max():.3e}, median {np.median(diffs):.3e}")
        assert diffs.max() <= steps * lr * 0.05 and np.median(diffs) <= steps * lr * 1e-4
    after = pol.forward(*data["cuda"], deterministic=True).loc
    assert not torch.equal(before, after)                       # no explicit refresh: the version counters moved
    new = {k: v.detach().cpu().numpy() for k, v in nets["cuda"][0].items()}
    newc = {k: v.detach().cpu().numpy() for k, v in nets["cuda"][1].items()}
    loc64 = R.forward(new, newc, obs, dtype=torch.float64)[0].numpy()
    assert np.abs(after.cpu().double().numpy() - loc64).max() < 1e-4


def test_device_refusals_raise_before_any_launch():
    actor, obs, action, lpo, adv, index = _case(48, 3, 5, 20, 811, B=20)
    d = lambda x: torch.as_tensor(x).cuda()
    c = {k: d(v) for k, v in actor.items()}
    xs, xo, xc, ad, ld, vd, idx = d(obs["state_self"]), d(obs["state_others"]), d(obs["cylinders"]), d(action), d(lpo), d(adv), d(index)
    with pytest.raises(ValueError, match="share one device"):                  # tensors on different devices
        AT.policy_loss_and_grad(c, xs, xo, xc, ad, ld, torch.as_tensor(adv), idx)
    with pytest.raises(ValueError, match="share one device"):
        AT.policy_loss_and_grad(c, xs, xo, xc, torch.as_tensor(action), ld, vd, idx)
    with pytest.raises(ValueError, match="share one device"):
        AT.policy_loss_and_grad(c, xs, xo, xc, ad, ld, vd, torch.as_tensor(index))
    with pytest.raises(ValueError, match="share one device"):
        AT.policy_loss_and_grad({**c, "act_dist.log_std": c["act_dist.log_std"].cpu()}, xs, xo, xc, ad, ld, vd, idx)
    with pytest.raises(ValueError, match="contiguous"):                        # a strided index would be read as consecutive int64
        AT.policy_loss_and_grad(c, xs, xo, xc, ad, ld, vd, torch.stack([idx, idx], dim=1)[:, 0])
    odd = torch.zeros(129, device="cuda")[1:]                                   # 4-byte aligned storage offset
    with pytest.raises(ValueError, match="16-byte aligned"):
        AT.policy_loss_and_grad({**c, "encoder.norm1.bias": odd.copy_(c["encoder.norm1.bias"])}, xs, xo, xc, ad, ld, vd, idx)
    c2 = {k: v.clone() for k, v in c.items()}
    c2["encoder.norm1.bias"].grad = torch.zeros(256, device="cuda")[::2]            # right shape and dtype, not contiguous
    with pytest.raises(ValueError, match="existing .grad"):
        AT.policy_loss_and_grad(c2, xs, xo, xc, ad, ld, vd, idx)
    assert all(v.grad is None for v in c.values())                              # nothing was launched or allocated on the refused calls
    out = AT.policy_loss_and_grad(c, xs, xo, xc, ad, ld, vd, idx)
    opt = AT.make_optimizer(c)
    with pytest.raises(ValueError, match="grad_norm"):
        opt.step()
    with pytest.raises(ValueError, match="grad_norm"):
        opt.step(grad_norm=out.grad_norm.cpu())
    before = {k: v.clone() for k, v in c.items()}
    opt.step(grad_norm=out.grad_norm)
    assert any(not torch.equal(before[k], c[k]) for k in c)


def test_report_ratios():
    print("actor gate ratios (worst per case):", RATIOS)
