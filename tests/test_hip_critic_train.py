"""The critic's update on the device (hns_critic_train_grad, hns_adam_clipped through hns_amd.critic_train) on an MI355X.

Accuracy gate (the rule of test_tp_train.py and test_hip_policy.py, BAR = 8): for value_loss, explained_var, the gradient norm and EACH of
the critic's gradient tensors, e_hip <= 8 max(e_32, 2^-24 max|g_64|), errors as max-abs against fp64 autograd of
tests/critic_update_reference.py, e_32 the error of the same statements in CPU torch fp32 autograd.  Every case asserts first, on the CPU,
that the two mean losses are at least 1e-3 of the loss apart in fp64, so no case sits on the tie of the max; a wrong branch moves every
gradient by far more than the bound.  Worst measured ratio per case: printed by test_report_ratios (RATIOS).

Measured on an MI355X (worst e_hip / max(e_32, 2^-24 max|ref_64|) over the three scalars, values and the 22 gradient tensors):
  fixture shapes: a3k5d35 1.82 / 2.08 (scaled returns) / 1.82 (mse), a3k8d20 1.74 / 1.57 / 1.74, a1k5d20 3.18 / 1.43 / 3.18,
  a6k16d24 1.84 / 1.46 / 1.84; branch-toward 2.21, branch-away 2.02; the recorded cases of g_critic_update.npz: a3k5d35 1.77, a3k8d20 4.11,
  a1k5d20 1.56, a6k16d24 2.12 (the recorded branch each time); the exact tie 4.35; 8 192 of the 131 072 env-steps of a [2048, 64] rollout 3.80 / 2.32;
  a full 65 536-env-step minibatch 3.92 (the gradient norm; every tensor <= 1.72); flat_tokens 1.96, saturated_softmax 4.86, large_obs 3.55;
  shape limits: A = 1 1.89, A = 7 1.29, K = 1 2.34, K = 16 1.88, D = 1 1.47, D = 96 1.77, one env-step 1.63, 33 rows 1.74.
  End to end (64 updates): max |device - cpu| 1.8e-4, median 1.9e-9."""
import math

import numpy as np
import pytest
import torch

import critic_update_reference as U
import policy_reference as R
from hns_amd import critic_train as CT
from hns_amd import policy as P

pytestmark = pytest.mark.gpu

BAR = 8.0
RATIOS = {}


def _net(D, A, seed, weight_scale=1.0, embed_scale=1.0, flat_bias=False):
    _, critic = P.random_parameters(D, A, seed)
    g = torch.Generator().manual_seed(seed + 7)
    for k, v in critic.items():
        if k.endswith("bias") or "norm" in k:
            critic[k] = v + torch.randn(v.shape, generator=g) * 0.1
        if "in_proj_weight" in k:
            critic[k] = critic[k] * weight_scale
        if "split_embed.embed" in k and k.endswith("weight"):
            critic[k] = critic[k] * embed_scale
        if k == "v_out.weight":
            critic[k] = v * 30.0                               # values of order 0.3: the clip at 0.1 cuts some rows and not others
    critic = {k: v.numpy().astype(np.float32) for k, v in critic.items()}
    if flat_bias:
        for k in critic:
            if "split_embed.embed" in k and k.endswith("bias"):
                critic[k] = (np.full_like(critic[k], 0.3) + np.linspace(0, 1e-3, critic[k].size, dtype=np.float32)).astype(np.float32)
    return critic


def _obs(S, A, K, D, seed, scale=1.0):
    g = np.random.default_rng(seed)
    obs = {"state_self": (g.standard_normal((S, A, 1, D)) * 0.7 * scale).astype(np.float32)}
    if A > 1:
        obs["state_others"] = (g.standard_normal((S, A, A - 1, 3)) * 0.5 * scale).astype(np.float32)
    obs["cylinders"] = (g.standard_normal((S, A, K, 5)) * 0.5 * scale).astype(np.float32)
    return obs


def _targets(critic, obs, seed, ret_scale=1.0, bv_noise=0.1, shift=None, chunk=4096):
    """b_values near the critic's own values (so the clip is active on part of the rows), returns around them.  `shift`: half of the rows
    instead get old values |shift| nearer to (+) or further from (-) the returns than the new ones, which decides the branch of the max."""
    S = obs["state_self"].shape[0]
    vals = []
    for s in range(0, S, chunk):
        o = {k: torch.as_tensor(v[s:s + chunk]) for k, v in obs.items()}
        p = {k: torch.as_tensor(v) for k, v in critic.items()}
        with torch.no_grad():
            vals.append(R._lin(R.encoder(p, "base.", o, torch.float32), p["v_out.weight"], p["v_out.bias"]).numpy())
    v = np.concatenate(vals)
    g = np.random.default_rng(seed)
    bv = (v + g.standard_normal(v.shape) * bv_noise).astype(np.float32)
    ret = ((v + g.standard_normal(v.shape)) * ret_scale).astype(np.float32)
    if shift is not None:
        half = g.random(v.shape) < 0.5
        bv = np.where(half, v + shift * np.sign(ret - v), v + (bv - v) * 0.3).astype(np.float32)
    return bv, ret


def _dev_call(critic, obs, bv, ret, index, shape=None, **kw):
    """Runs value_loss_and_grad on the device; obs as [S, A, ..] (flat) or, with shape = (N, T), as the [N, T, A, ..] rollout."""
    c = {k: torch.as_tensor(v).cuda() for k, v in critic.items()}
    def lay(x):
        t = torch.as_tensor(x).cuda()
        return t.reshape(*shape, *t.shape[1:]) if shape else t
    xs, xc = lay(obs["state_self"]), lay(obs["cylinders"])
    xo = lay(obs["state_others"]) if "state_others" in obs else None
    idx = torch.as_tensor(np.asarray(index)).cuda() if index is not None else None
    out = CT.value_loss_and_grad(c, xs, xo, xc, lay(bv), lay(ret), idx, **kw)
    torch.cuda.synchronize()
    return c, out


def _ref_chunked(critic, obs, bv, ret, index, dtype, **kw):
    return U.loss_and_grad(critic, obs, bv, ret, index, dtype=dtype, **kw)


def gate(tag, critic, obs, bv, ret, index, shape=None, tie=False, **kw):
    r64 = _ref_chunked(critic, obs, bv, ret, index, torch.float64, **kw)
    r32 = _ref_chunked(critic, obs, bv, ret, index, torch.float32, **kw)
    sep = abs(r64["l_orig"] - r64["l_clip"])
    if tie:
        assert r64["branch"] == 2 and r32["branch"] == 2, f"{tag}: not an exact tie"
    else:
        assert sep >= 1e-3 * r64["value_loss"], f"{tag}: the two mean losses are {sep:.3e} apart: the case sits on the tie"
    c, out = _dev_call(critic, obs, bv, ret, index, shape, **kw)
    worst, bad = 0.0, []
    items = [(n, float(getattr(out, n)), r64[n], r32[n]) for n in ("value_loss", "explained_var", "grad_norm")]
    items += [(n, c[n].grad.cpu().double().numpy(), r64["grads"][n], r32["grads"][n]) for n in r64["grads"]]
    items.append(("values", out.values.cpu().double().numpy(), r64["values"], r32["values"]))
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
    RATIOS[tag] = (worst, r64["branch"])
    assert not bad, f"{tag}: " + "; ".join(bad)
    return r64


def _case(S, A, K, D, seed, B=None, ret_scale=1.0, bv_noise=0.1, obs_scale=1.0, shift=None, **net):
    critic = _net(D, A, seed, **net)
    obs = _obs(S, A, K, D, seed + 1, obs_scale)
    bv, ret = _targets(critic, obs, seed + 2, ret_scale, bv_noise, shift)
    index = np.random.default_rng(seed + 3).permutation(S)[:B] if B else None
    return critic, obs, bv, ret, index


@pytest.mark.parametrize("shape", [(3, 5, 35), (3, 8, 20), (1, 5, 20), (6, 16, 24)])
@pytest.mark.parametrize("variant", ["huber", "far_returns", "mse"])
def test_fixture_shapes_pass_the_fp64_gate(shape, variant):
    """The four shapes of g_policy.npz with a strict shuffled subset of the env-steps as the index: Huber, returns scaled so that the
    gradient norm exceeds max_grad_norm 10 and rows leave the Huber delta, and MSE."""
    A, K, D = shape
    kw = {"loss": "mse"} if variant == "mse" else {}
    far = variant == "far_returns"
    critic, obs, bv, ret, index = _case(48, A, K, D, 100 + A + K, B=37, ret_scale=40.0 if far else 1.0, shift=(0.5 if K == 5 else -0.5) if far else None)
    gate(f"a{A}k{K}d{D}-{variant}", critic, obs, bv, ret, index, **kw)


def test_both_branches_of_the_max_occur():
    """Half of the rows with old values 0.3 nearer to the returns than the new ones (the unclipped loss is the larger mean), then 0.3 further
    (the clipped one is); the other half stays inside the clip and carries the gradient in the second case."""
    seen = set()
    for name, shift in (("toward", +0.3), ("away", -0.3)):
        critic, obs, bv, ret, index = _case(64, 3, 5, 35, 301, B=50, shift=shift)
        seen.add(gate(f"branch-{name}", critic, obs, bv, ret, index)["branch"])
    assert seen == {0, 1}, seen


@pytest.mark.parametrize("tag", ["a3k5d35", "a3k8d20", "a1k5d20", "a6k16d24"])
def test_golden_fixture_cases_pass_the_fp64_gate(tag):
    """The cases of g_critic_update.npz (the reference's own update_critic, recorded): the gate against fp64, the branch the reference
    recorded, and the device's scalars and clipped-before gradients within the gate's bound of the recorded fp32 ones by construction."""
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    critic, obs, bv, ret, index, loss, rec = U.golden_case(np.load(os.path.join(here, "g_critic_update.npz")), np.load(os.path.join(here, "g_policy.npz")), tag)
    r = gate(f"golden-{tag}", critic, obs, bv, ret, index, loss=loss)
    assert r["branch"] == int(rec["branch"])
    c, out = _dev_call(critic, obs, bv, ret, index, loss=loss)
    lo, lc = float(rec["u1:l_orig"]), float(rec["u1:l_clip"])
    assert abs(float(out.value_loss) - max(lo, lc)) <= 1e-5 * max(lo, lc)            # the recorded larger mean, not the other one
    assert abs(float(out.value_loss) - min(lo, lc)) > 1e-4 * max(lo, lc)
    assert abs(float(out.grad_norm) - float(rec["u1:grad_norm"])) <= 1e-4 * float(rec["u1:grad_norm"])


def test_exact_tie_gives_each_branch_half():
    """b_values = 0 and a clip wider than every |v|: clipped = 0 + (v - 0) = v bit for bit in every precision, the two means are the same
    number, and torch.maximum's backward gives each branch half — the (1/2, 1/2) weights of hns_critic_loss_kernel."""
    critic, obs, bv, ret, index = _case(64, 3, 5, 35, 331, B=50)
    gate("tie", critic, obs, np.zeros_like(bv), ret, index, tie=True, clip_param=100.0)


@pytest.mark.parametrize("seed", [411, 412])
def test_random_minibatches_pass_the_fp64_gate(seed):
    """A rollout of 2 048 envs x 64 steps read in place, an index of 8 192 of its 131 072 env-steps (24 576 rows: the reference default
    minibatch); the fp64 yardstick gathers the minibatch first, so only it is held in fp64."""
    critic, obs, bv, ret, index = _case(2048 * 64, 3, 5, 35, seed, B=8192)
    assert index.max() > 2 ** 16
    gate(f"random-{seed}", critic, obs, bv, ret, index, shape=(2048, 64))


def test_full_65536_env_minibatch_passes_the_fp64_gate():
    """'One full 65 536-env minibatch' read as 65 536 env-steps (196 608 rows) without an index; the fp64 yardstick runs in chunks of 8 192
    env-steps (tests/critic_update_reference.py).  The cost tool's 65 536-env rollout has minibatches of 262 144 env-steps: the same kernels on
    four times the tiles, not gated here (the CPU yardstick alone would take several minutes)."""
    critic, obs, bv, ret, index = _case(65536, 3, 5, 35, 421)
    gate("full-65536", critic, obs, bv, ret, None)


@pytest.mark.parametrize("mode", ["flat_tokens", "saturated_softmax", "large_obs"])
def test_numerical_edges_pass_the_fp64_gate(mode):
    """test_hip_policy.py's three edges; LayerNorm's backward divides by the standard deviation, so flat tokens are where a wrong formulation shows."""
    if mode == "flat_tokens":
        critic, obs, bv, ret, index = _case(1024, 3, 8, 20, 21, B=700, embed_scale=1e-4, flat_bias=True)
    elif mode == "saturated_softmax":
        critic, obs, bv, ret, index = _case(1024, 3, 8, 20, 22, B=700, weight_scale=40.0)
    else:
        critic, obs, bv, ret, index = _case(1024, 3, 8, 20, 23, B=700, obs_scale=300.0)
    gate(mode, critic, obs, bv, ret, index)


@pytest.mark.parametrize("shape", [(1, 5, 20, 40), (7, 5, 20, 9), (3, 1, 20, 33), (3, 16, 20, 33), (3, 5, 1, 33), (3, 5, 96, 33), (3, 5, 35, 1), (3, 5, 35, 11)])
def test_shape_limits(shape):
    """A = 1 and 7, K = 1 and 16, self_dim 1 and 96, a minibatch of one env-step and one whose row count is not a multiple of 32."""
    A, K, D, B = shape
    critic, obs, bv, ret, index = _case(48, A, K, D, 500 + A + K + D + B, B=B, shift=-0.3 if B % 2 else 0.3)
    gate(f"limit-a{A}k{K}d{D}b{B}", critic, obs, bv, ret, index)


def _grads(c):
    return {k: v.grad.clone() for k, v in c.items()}


def test_bit_identity_across_calls_index_layout_and_graph_replay():
    critic, obs, bv, ret, index = _case(32 * 16, 3, 5, 35, 611, B=300)
    c1, o1 = _dev_call(critic, obs, bv, ret, index, shape=(32, 16))
    c2, o2 = _dev_call(critic, obs, bv, ret, index, shape=(32, 16))
    g1 = _grads(c1)
    for k in g1:
        assert torch.equal(g1[k], c2[k].grad), k
    for n in ("value_loss", "explained_var", "grad_norm", "values"):
        assert torch.equal(getattr(o1, n), getattr(o2, n)), n
    # the index against an explicit gather, [N, T, ..] strided against flat contiguous; a strided index made contiguous reads the same rows
    c5, o5 = _dev_call(critic, obs, bv, ret, np.ascontiguousarray(np.stack([index, index[::-1]], axis=1)[:, 0]), shape=(32, 16))
    assert all(torch.equal(g1[k], c5[k].grad) for k in g1)
    gathered = {k: v[index] for k, v in obs.items()}
    c3, o3 = _dev_call(critic, gathered, bv[index], ret[index], None)
    for k in g1:
        assert torch.equal(g1[k], c3[k].grad), k
    assert torch.equal(o1.value_loss, o3.value_loss) and torch.equal(o1.values, o3.values) and torch.equal(o1.grad_norm, o3.grad_norm)
    wide = {k: np.concatenate([v, np.zeros_like(v)], axis=-1) for k, v in obs.items()}       # a view with strides: the last dim cut from twice the width
    c = {k: torch.as_tensor(v).cuda() for k, v in critic.items()}
    lay = lambda x: torch.as_tensor(x).cuda().reshape(32, 16, *x.shape[1:])
    xs, xo, xc = (lay(wide[k])[..., :obs[k].shape[-1]] for k in ("state_self", "state_others", "cylinders"))
    assert not xs.is_contiguous()
    idx = torch.as_tensor(index).cuda()
    o4 = CT.value_loss_and_grad(c, xs, xo, xc, lay(bv), lay(ret), idx)
    for k in g1:
        assert torch.equal(g1[k], c[k].grad), k
    assert torch.equal(o1.value_loss, o4.value_loss)
    # eager against one replay of a single-stream capture of value_loss_and_grad + step
    def fresh():
        cc = {k: torch.as_tensor(v).cuda() for k, v in critic.items()}
        return cc, CT.ClippedAdam(cc.values(), lr=5e-4, max_grad_norm=10.0)
    ce, oe = fresh()
    xs, xo, xc = (lay(obs[k]) for k in ("state_self", "state_others", "cylinders"))
    bvd, retd = lay(bv), lay(ret)
    for _ in range(2):
        out = CT.value_loss_and_grad(ce, xs, xo, xc, bvd, retd, idx)
        oe.step(grad_norm=out.grad_norm)
    cg, og = fresh()
    out = CT.value_loss_and_grad(cg, xs, xo, xc, bvd, retd, idx)          # eager first step: allocates .grad and the optimizer state
    og.step(grad_norm=out.grad_norm)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = CT.value_loss_and_grad(cg, xs, xo, xc, bvd, retd, idx, check_index=False)
        og.step(grad_norm=out.grad_norm)
    graph.replay()
    torch.cuda.synchronize()
    for k in ce:
        assert torch.equal(ce[k], cg[k]), k
    assert float(next(iter(og.state.values()))["step"]) == 2.0


@pytest.mark.parametrize("max_norm", [10.0, 1e9, float("inf")])
def test_adam_clipped_matches_the_numpy_restatement_bit_for_bit(max_norm):
    """22 tensors, one step-counter bump per call, the clip active (norm ~ 40 > 10), inactive (1e9) and off (inf)."""
    g = np.random.default_rng(7)
    shapes = [(128, 35), (128,), (128, 3), (128,), (128, 5), (128,), (128,), (128,), (384, 128), (384,), (128, 128), (128,), (128, 128), (128,),
              (128, 128), (128,), (128,), (128,), (128,), (128,), (1, 128), (1,)]
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
        ps, cg, ms, vs, step = U.clip_adam_np(ps, gs, ms, vs, step, norm, max_norm)
        torch.cuda.synchronize()
        for k, (p, x) in enumerate(zip(dev, ps)):
            assert np.array_equal(p.detach().cpu().numpy(), x), (it, k)
            assert np.array_equal(p.grad.cpu().numpy(), cg[k]), (it, k)                  # the gradients hold the clipped values, as torch leaves them
            assert np.array_equal(opt.state[p]["exp_avg"].cpu().numpy(), ms[k]) and np.array_equal(opt.state[p]["exp_avg_sq"].cpu().numpy(), vs[k])
        assert float(opt.state[dev[0]]["step"]) == it + 1 == float(step)


@pytest.mark.parametrize("max_norm", [1.0, float("inf")])
def test_adam_clipped_over_65_tensors_steps_both_launches_with_one_count(max_norm):
    """65 tensors of 3 to 40 values: one past the 64 descriptors a launch carries, so the second launch of a step runs while the counter is
    still unbumped.  Two steps, bit for bit against the restatement (which uses ONE step + 1 for all tensors), with the clip active (the norm
    is ~ 4 to 40 > 1) and off; the counter reads 2.0."""
    g = np.random.default_rng(65)
    sizes = [3 + (7 * k) % 38 for k in range(65)]
    assert min(sizes) == 3 and max(sizes) == 40 and len(sizes) == 65
    ps = [g.standard_normal(n).astype(np.float32) for n in sizes]
    ms, vs, step = [np.zeros(n, np.float32) for n in sizes], [np.zeros(n, np.float32) for n in sizes], np.float32(0)
    dev = [torch.nn.Parameter(torch.as_tensor(p).cuda()) for p in ps]
    opt = CT.ClippedAdam(dev, lr=5e-4, max_grad_norm=max_norm)
    for it in range(2):
        gs = [(g.standard_normal(n) * 10.0 ** (it - 1)).astype(np.float32) for n in sizes]
        norm = np.float32(math.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for x in gs)))
        assert norm > 1.0
        for p, x in zip(dev, gs):
            p.grad = torch.as_tensor(x).cuda()
        opt.step(grad_norm=torch.tensor(norm, device="cuda"))
        ps, cg, ms, vs, step = U.clip_adam_np(ps, gs, ms, vs, step, norm, max_norm)
        for k, (p, x) in enumerate(zip(dev, ps)):
            assert np.array_equal(p.detach().cpu().numpy(), x), (it, k)
            assert np.array_equal(p.grad.cpu().numpy(), cg[k]), (it, k)
            assert np.array_equal(opt.state[p]["exp_avg"].cpu().numpy(), ms[k]) and np.array_equal(opt.state[p]["exp_avg_sq"].cpu().numpy(), vs[k]), (it, k)
    assert all(opt.state[p]["step"] is opt.state[dev[0]]["step"] for p in dev)
    assert float(opt.state[dev[0]]["step"]) == 2.0 == float(step)


def test_update_critic_end_to_end_and_the_policy_follows():
    """Four epochs x 16 minibatches from the same start and the same permutations on the device and in CPU torch.  Bound: Adam moves a
    parameter by at most ~lr per step whatever the gradient's size, and a gradient error of relative size r near |g| ~ sqrt(v) moves the step
    by ~lr r; with the gate's per-gradient error (<= 8 x fp32 autograd's own, itself ~1e-6 relative on these tensors) the drift is
    ~lr 1e-5 per step; where |g| is at rounding level the step's direction is arbitrary on both sides, bounded by lr per step.  So: every
    parameter within 64 steps x lr x 0.05 = 1.6e-3 absolute, and the median |difference| at most 64 x lr x 1e-4 = 3.2e-6."""
    critic, obs, bv, ret, _ = _case(16 * 32, 3, 5, 35, 711)
    S = 16 * 32
    cpu = {k: torch.nn.Parameter(torch.as_tensor(v)) for k, v in critic.items()}
    dev = {k: torch.nn.Parameter(torch.as_tensor(v).cuda()) for k, v in critic.items()}
    oc, od = CT.make_optimizer(cpu), CT.make_optimizer(dev)
    actor, _ = P.random_parameters(35, 3, 5)
    pol = P.DevicePolicy({k: v.cuda() for k, v in actor.items()}, dev)
    t = lambda x, d: torch.as_tensor(x).to(d)
    xs_d = t(obs["state_self"], "cuda")
    before = pol.forward(xs_d, t(obs["state_others"], "cuda"), t(obs["cylinders"], "cuda"), value_only=True).value.clone()
    gen = torch.Generator().manual_seed(3)
    for _ in range(4):
        perm = torch.randperm(S, generator=gen).reshape(16, -1)
        for idx in perm:
            for params, opt, d in ((cpu, oc, "cpu"), (dev, od, "cuda")):
                st = CT.update_critic(params, t(obs["state_self"], d), t(obs["state_others"], d), t(obs["cylinders"], d), t(bv, d), t(ret, d), opt,
                                      index=idx.to(d))
                assert st["value_loss"].dim() == 0 and st["value_loss"].device.type == d
    lr, steps = 5e-4, 64
    diffs = np.concatenate([(dev[k].detach().cpu() - cpu[k].detach()).abs().numpy().ravel() for k in cpu])
    print(f"  end to end: max |dev - cpu| {diffs.max():.3e}, median {np.median(diffs):.3e}")
    assert diffs.max() <= steps * lr * 0.05 and np.median(diffs) <= steps * lr * 1e-4
    after = pol.forward(xs_d, t(obs["state_others"], "cuda"), t(obs["cylinders"], "cuda"), value_only=True).value
    assert not torch.equal(before, after)                       # no explicit refresh: the version counters moved
    new = {k: v.detach().cpu().numpy() for k, v in dev.items()}
    o = {k: torch.as_tensor(v) for k, v in obs.items()}
    p = {k: torch.as_tensor(v) for k, v in new.items()}
    with torch.no_grad():
        v64 = R._lin(R.encoder(p, "base.", o, torch.float64), p["v_out.weight"].double(), p["v_out.bias"].double()).numpy()
    assert np.abs(after.cpu().double().numpy() - v64).max() < 1e-4


def test_device_refusals_raise_before_any_launch():
    critic, obs, bv, ret, index = _case(48, 3, 5, 20, 811, B=20)
    d = lambda x: torch.as_tensor(x).cuda()
    c = {k: d(v) for k, v in critic.items()}
    xs, xo, xc, bvd, retd, idx = d(obs["state_self"]), d(obs["state_others"]), d(obs["cylinders"]), d(bv), d(ret), d(index)
    with pytest.raises(ValueError, match="share one device"):                  # tensors on different devices
        CT.value_loss_and_grad(c, xs, xo, xc, bvd, torch.as_tensor(ret), idx)
    with pytest.raises(ValueError, match="share one device"):
        CT.value_loss_and_grad(c, xs, xo, xc, bvd, retd, torch.as_tensor(index))
    with pytest.raises(ValueError, match="share one device"):
        CT.value_loss_and_grad({**c, "v_out.bias": c["v_out.bias"].cpu()}, xs, xo, xc, bvd, retd, idx)
    with pytest.raises(ValueError, match="contiguous"):                        # a strided index would be read as consecutive int64
        CT.value_loss_and_grad(c, xs, xo, xc, bvd, retd, torch.stack([idx, idx], dim=1)[:, 0])
    odd = torch.zeros(129, device="cuda")[1:]                                   # 4-byte aligned storage offset
    with pytest.raises(ValueError, match="16-byte aligned"):
        CT.value_loss_and_grad({**c, "base.norm1.bias": odd.copy_(c["base.norm1.bias"])}, xs, xo, xc, bvd, retd, idx)
    c2 = {k: v.clone() for k, v in c.items()}
    c2["base.norm1.bias"].grad = torch.zeros(256, device="cuda")[::2]               # right shape and dtype, not contiguous
    with pytest.raises(ValueError, match="existing .grad"):
        CT.value_loss_and_grad(c2, xs, xo, xc, bvd, retd, idx)
    assert all(v.grad is None for v in c.values())                              # nothing was launched or allocated on the refused calls
    out = CT.value_loss_and_grad(c, xs, xo, xc, bvd, retd, idx)
    opt = CT.ClippedAdam(c.values(), max_grad_norm=10.0)
    with pytest.raises(ValueError, match="grad_norm"):
        opt.step()
    with pytest.raises(ValueError, match="grad_norm"):
        opt.step(grad_norm=out.grad_norm.cpu())
    before = {k: v.clone() for k, v in c.items()}
    opt.step(grad_norm=out.grad_norm)
    assert any(not torch.equal(before[k], c[k]) for k in c)


def test_report_ratios():
    print("critic gate ratios (worst, branch):", {k: (round(v[0], 2), v[1]) for k, v in RATIOS.items()})
