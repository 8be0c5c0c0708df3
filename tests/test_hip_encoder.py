"""The encoder as a differentiable op on the device (hns_encoder_forward / hns_encoder_backward through hns_amd.encoder) on an MI355X.

Accuracy gate (the rule of test_hip_critic_train.py, test_tp_train.py and test_hip_policy.py, BAR = 8): for the features and for EACH of the
encoder's 20 gradient tensors, e_hip <= 8 max(e_32, 2^-24 max|ref_64|), errors as max-abs against tests/policy_reference.py's encoder in
fp64 (the gradients: fp64 autograd of (encoder(...) * dy).sum() with a seeded normal dy), e_32 the error of the same statements in CPU fp32.
Every backward case asserts first, on the CPU, that no fp64 reference gradient tensor is identically zero; in_proj_bias' k third, which the
softmax cancels, must be exactly zero on the device.  Worst measured ratio per case: printed by test_report_ratios (RATIOS).
The backward pass's own plan (train_plan): tiles of kEncRows = 32 rows, tps = ceil(tiles / kCtMaxSplits) tiles per row range of the weight-gradient
kernel, kCtMaxSplits = 48.  523 env-steps x 3 agents = 1 569 rows = 50 tiles: tps 2, 25 splits, one live row in the last tile — the one shape
that takes the tps > 1 branch through hns_encoder_backward and hns_encoder_reduce_kernel (asserted from these constants).

Measured on an MI355X (worst e_hip / max(e_32, 2^-24 max|ref_64|) over a case's tensors; features / the 20 gradient tensors):
  fixture shapes: a3k5d35 0.76 / 1.03, a3k8d20 1.08 / 1.41, a1k5d20 0.83 / 1.86, a6k16d24 1.40 / 1.61;
  shape limits: A = 1 1.02 / 1.39, A = 7 0.83 / 1.43, K = 1 1.11 / 1.34, K = 16 1.22 / 1.66, D = 1 0.95 / 1.12, D = 96 1.00 / 1.27,
  one env-step 1.35 / 2.12, 33 rows 1.22 / 1.46; past 48 weight-gradient tiles (523 env-steps x 3 agents: 50 tiles, two per split) 0.90 / 1.29;
  the custom critic end to end (value_loss, values, the head's and the encoder's gradients): the op path 1.96 (unclipped branch) and 1.36
  (clipped branch), the fused value_loss_and_grad on the same inputs 1.86 and 1.62."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import critic_update_reference as U
import policy_reference as R
from hns_amd import abi
from hns_amd import critic_train as CT
from hns_amd import encoder as EN
from hns_amd import policy as P
from hns_amd import policy_train as PT

pytestmark = pytest.mark.gpu

BAR = 8.0
RATIOS = {}
# (A, K, D, env-steps): the four fixture shapes of g_policy.npz, then one value at its limit per case: A = 1 (no state_others) and 7, K = 1 and
# 16, D = 1 and 96, one env-step, 11 env-steps x 3 agents = 33 rows (the second tile has a single live row); PAST_SPLITS: more tiles than the
# weight-gradient kernel has row ranges (test_the_large_shape_takes_two_tiles_per_split)
PAST_SPLITS = (3, 5, 35, 523)
SHAPES = [(3, 5, 35, 37), (3, 8, 20, 37), (1, 5, 20, 37), (6, 16, 24, 37),
          (1, 5, 20, 40), (7, 5, 20, 9), (3, 1, 20, 33), (3, 16, 20, 33), (3, 5, 1, 33), (3, 5, 96, 33), (3, 5, 35, 1), (3, 5, 35, 11), PAST_SPLITS]
CANARY = 1234.5
ROWS, MAX_SPLITS = 32, 48                                       # csrc/hns_encoder.h: kEncRows; csrc/hns_policy_train.hip: kCtMaxSplits


def test_the_large_shape_takes_two_tiles_per_split():
    """hns_encoder_backward's own plan (train_plan): tiles of 32 rows, tps = ceil(tiles / 48) tiles per split.  Every other shape of SHAPES has
    at most 7 tiles (tps 1); PAST_SPLITS is the smallest A = 3 batch with tps 2 whose last tile holds ONE live row: 1 569 rows, 50 tiles, 25
    splits."""
    plan = lambda rows: (-(-rows // ROWS), -(-(-(-rows // ROWS)) // MAX_SPLITS))
    A, _, _, S = PAST_SPLITS
    rows = S * A
    tiles, tps = plan(rows)
    assert (rows, tiles, tps, -(-tiles // tps)) == (1569, 50, 2, 25) and tiles > MAX_SPLITS
    assert rows - (tiles - 1) * ROWS == 1
    assert all(plan(s[3] * s[0])[1] == 1 and plan(s[3] * s[0])[0] <= 7 for s in SHAPES if s != PAST_SPLITS)
    assert all(plan(r)[1] == 1 or r - (plan(r)[0] - 1) * ROWS != 1 for r in range(A, rows, A))       # the smallest such batch


def _tag(shape):
    return "a%dk%dd%ds%d" % tuple(shape)


def _fields(critic):
    return {f: torch.as_tensor(critic["base." + k]) for k, f in P._ENCODER.items() if "base." + k in critic}


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """One network and batch per shape with its fp64 and fp32 references, computed once and shared by the forward and the backward gate:
    (critic by reference name, obs, dy, {dtype: (features, {field: gradient})})."""
    A, K, D, S = shape
    actor, critic, obs, _ = R.limit_case((A, K, D, S))
    dy = torch.randn(S, A, 128, generator=torch.Generator().manual_seed(1000 + S + A))
    o = {k: torch.as_tensor(v) for k, v in obs.items()}
    refs = {}
    for dtype in (torch.float64, torch.float32):
        q = {k: torch.as_tensor(v).to(dtype).requires_grad_(True) for k, v in critic.items() if k.startswith("base.")}
        y = R.encoder(q, "base.", o, dtype)
        (y * dy.to(dtype)).sum().backward()
        refs[dtype] = (y.detach().double().numpy(), {P._ENCODER[k[len("base."):]]: v.grad.double().numpy() for k, v in q.items()})
    return critic, obs, dy, refs


def _dev(critic, obs, requires_grad=True):
    p = {f: t.cuda().requires_grad_(requires_grad) for f, t in _fields(critic).items()}
    xs, xc = torch.as_tensor(obs["state_self"]).cuda(), torch.as_tensor(obs["cylinders"]).cuda()
    xo = torch.as_tensor(obs["state_others"]).cuda() if "state_others" in obs else None
    return p, xs, xo, xc


def _gate(tag, items):
    """items: (name, device value, fp64 reference, fp32 reference); records the worst ratio under `tag` and asserts the bar."""
    worst, bad = 0.0, []
    for name, h, a, b in items:
        h, a, b = np.asarray(h, np.float64), np.asarray(a, np.float64), np.asarray(b, np.float64)
        assert h.shape == a.shape == b.shape, (name, h.shape, a.shape)
        assert np.isfinite(h).all(), f"{tag} {name}: not finite"
        e_hip, e_32 = float(np.abs(h - a).max()), float(np.abs(b - a).max())
        bound = max(e_32, 2.0 ** -24 * float(np.abs(a).max()))
        ratio = e_hip / bound if bound > 0 else (0.0 if e_hip == 0 else math.inf)
        print(f"  {tag} {name}: e_hip {e_hip:.3e} e_32 {e_32:.3e} max|ref| {np.abs(a).max():.3e} ratio {ratio:.2f}")
        worst = max(worst, ratio)
        if not ratio <= BAR:
            bad.append(f"{name}: e_hip {e_hip:.3e} > {BAR} x {bound:.3e} (ratio {ratio:.2f})")
    RATIOS[tag] = max(worst, RATIOS.get(tag, 0.0))
    assert not bad, f"{tag}: " + "; ".join(bad)


@pytest.mark.parametrize("shape", SHAPES, ids=_tag)
def test_features_pass_the_fp64_gate(shape):
    critic, obs, _, refs = _reference(shape)
    p, xs, xo, xc = _dev(critic, obs, requires_grad=False)
    feats = EN.encode(p, xs, xo, xc)
    assert tuple(feats.shape) == (shape[3], shape[0], 128) and feats.dtype == torch.float32
    _gate("fwd-" + _tag(shape), [("features", feats.cpu().numpy(), refs[torch.float64][0], refs[torch.float32][0])])


@pytest.mark.parametrize("shape", SHAPES, ids=_tag)
def test_gradients_pass_the_fp64_gate(shape):
    critic, obs, dy, refs = _reference(shape)
    g64, g32 = refs[torch.float64][1], refs[torch.float32][1]
    assert len(g64) == (20 if shape[0] > 1 else 18)
    for f, g in g64.items():
        assert g.any(), f"{f}: the fp64 reference gradient is identically zero, the case gates nothing"
    assert not np.abs(g64["in_proj_b"][128:256]).max() > 1e-12
    p, xs, xo, xc = _dev(critic, obs)
    (EN.encode(p, xs, xo, xc) * dy.cuda()).sum().backward()
    assert set(p) == set(g64)
    _gate("bwd-" + _tag(shape), [(f, p[f].grad.cpu().numpy(), g64[f], g32[f]) for f in p])
    assert not p["in_proj_b"].grad[128:256].any(), "in_proj_bias' k third must be exactly zero"


def _targets(values, seed, shift):
    """b_values and returns around the critic's own values: half of the rows with old values |shift| nearer to (+) or further from (-) the returns
    than the new ones, which puts the two mean losses apart; the rest inside the clip."""
    g = np.random.default_rng(seed)
    bv = values + g.standard_normal(values.shape) * 0.1
    ret = values + g.standard_normal(values.shape)
    half = g.random(values.shape) < 0.5
    bv = np.where(half, values + shift * np.sign(ret - values), values + (bv - values) * 0.3)
    return bv.astype(np.float32), ret.astype(np.float32)


@pytest.mark.parametrize("shift", [0.3, -0.3])
def test_custom_critic_end_to_end_describes_the_fused_update_s_network(shift):
    """The op, a torch nn.Linear(128, 1), the reference's clipped value loss in torch and .backward(): every encoder and head gradient against
    update_critic in fp64 (critic_update_reference.loss_and_grad, off the tie of the max by its own separation assert) — and the fused
    value_loss_and_grad on the same inputs through the same gate: the two paths describe one network."""
    A, K, D, S, B = 3, 5, 35, 64, 50
    _, critic = R.random_net(D, A, 301)
    critic["v_out.weight"] = critic["v_out.weight"] * 30.0     # values of order 0.3: the clip at 0.1 cuts some rows and not others
    obs, _ = R.random_obs(S, A, K, D, 302)
    o = {k: torch.as_tensor(v) for k, v in obs.items()}
    q = {k: torch.as_tensor(v) for k, v in critic.items()}
    with torch.no_grad():
        v = R._lin(R.encoder(q, "base.", o, torch.float32), q["v_out.weight"], q["v_out.bias"]).numpy()
    bv, ret = _targets(v, 303, shift)
    index = np.random.default_rng(304).permutation(S)[:B]
    r64 = U.loss_and_grad(critic, obs, bv, ret, index, dtype=torch.float64)
    r32 = U.loss_and_grad(critic, obs, bv, ret, index, dtype=torch.float32)
    sep = abs(r64["l_orig"] - r64["l_clip"])
    assert sep >= 1e-3 * r64["value_loss"], f"the two mean losses are {sep:.3e} apart: the case sits on the tie"
    names = {f: "base." + k for k, f in P._ENCODER.items()}

    # the op path
    p, xs, xo, xc = _dev(critic, obs)
    head = nn.Linear(128, 1).cuda()
    with torch.no_grad():
        head.weight.copy_(torch.as_tensor(critic["v_out.weight"]))
        head.bias.copy_(torch.as_tensor(critic["v_out.bias"]))
    idx = torch.as_tensor(index).cuda()
    bvd, retd = torch.as_tensor(bv).cuda()[idx], torch.as_tensor(ret).cuda()[idx]
    values = head(EN.encode(p, xs.unsqueeze(0), xo.unsqueeze(0), xc.unsqueeze(0), idx))
    clipped = bvd + (values - bvd).clamp(-0.1, 0.1)
    loss_fn = nn.HuberLoss(delta=10.0)
    value_loss = torch.max(loss_fn(retd, values), loss_fn(retd, clipped))
    value_loss.backward()
    items = [("value_loss", value_loss.item(), r64["value_loss"], r32["value_loss"]),
             ("values", values.detach().cpu().numpy(), r64["values"], r32["values"]),
             ("v_out.weight", head.weight.grad.cpu().numpy(), r64["grads"]["v_out.weight"], r32["grads"]["v_out.weight"]),
             ("v_out.bias", head.bias.grad.cpu().numpy(), r64["grads"]["v_out.bias"], r32["grads"]["v_out.bias"])]
    items += [(f, p[f].grad.cpu().numpy(), r64["grads"][names[f]], r32["grads"][names[f]]) for f in p]
    _gate(f"custom-critic-op{shift:+.1f}", items)

    # the fused path on the same inputs
    c = {k: torch.as_tensor(v).cuda() for k, v in critic.items()}
    out = CT.value_loss_and_grad(c, xs.unsqueeze(0), xo.unsqueeze(0), xc.unsqueeze(0), torch.as_tensor(bv).cuda(), torch.as_tensor(ret).cuda(), idx)
    items = [("value_loss", float(out.value_loss), r64["value_loss"], r32["value_loss"]),
             ("values", out.values.cpu().numpy(), r64["values"], r32["values"])]
    items += [(n, c[n].grad.cpu().numpy(), r64["grads"][n], r32["grads"][n]) for n in r64["grads"]]
    _gate(f"custom-critic-fused{shift:+.1f}", items)


def _run(p, xs, xo, xc, index, dy):
    """features and gradients of one forward + backward on fresh leaves."""
    leaves = {f: t.detach().clone().requires_grad_(True) for f, t in p.items()}
    feats = EN.encode(leaves, xs, xo, xc, index)
    (feats * dy).sum().backward()
    torch.cuda.synchronize()
    return feats.detach(), {f: t.grad for f, t in leaves.items()}


def test_rollout_layouts_equal_the_flat_gathered_call_bit_for_bit():
    N, T, A, K, D, B = 8, 6, 3, 5, 35, 37
    _, critic = R.random_net(D, A, 611)
    obs, _ = R.random_obs(N * T, A, K, D, 612)
    p, xs, xo, xc = _dev(critic, obs, requires_grad=False)
    index = torch.as_tensor(np.random.default_rng(613).permutation(N * T)[:B]).cuda()
    assert B < N * T and not torch.equal(index, index.sort().values)
    dy = torch.randn(B, A, 128, generator=torch.Generator().manual_seed(614)).cuda()
    f0, g0 = _run(p, xs[index], xo[index], xc[index], None, dy)                # flat, gathered
    lay = lambda t: t.reshape(N, T, *t.shape[1:])
    f1, g1 = _run(p, lay(xs), lay(xo), lay(xc), index, dy)                    # the rollout read in place
    wide = [torch.full((N, 2 * T, *t.shape[1:]), float("nan"), device="cuda") for t in (xs, xo, xc)]
    for w, t in zip(wide, (xs, xo, xc)):
        w[:, :T] = lay(t)
    views = [w[:, :T] for w in wide]                                          # a slice of a wider [N, 2 T] rollout
    assert not any(v.is_contiguous() for v in views)
    f2, g2 = _run(p, *views, index, dy)
    for f, g in ((f1, g1), (f2, g2)):
        assert torch.equal(f, f0)
        for k in g0:
            assert torch.equal(g[k], g0[k]), k


def test_determinism_workspace_independence_and_canaries():
    A, K, D, S = 3, 5, 35, 21                                                 # 63 rows: the second tile is one row short
    _, critic = R.random_net(D, A, 711)
    obs, _ = R.random_obs(S, A, K, D, 712)
    p, xs, xo, xc = _dev(critic, obs, requires_grad=False)
    xs4, xo4, xc4 = PT.as_rollout(xs, xo, xc)
    shape = PT.validate("encoder", p, xs4, xo4, xc4, (), None, True)
    lib = abi.load_library()
    rows, E = S * A, 128
    nb = lib.hns_encoder_workspace_bytes(rows, D, A, K, 1)
    assert lib.hns_encoder_workspace_bytes(rows, D, A, K, 0) < nb
    dy = torch.randn(S, A, E, generator=torch.Generator().manual_seed(713)).cuda()
    offsets, n = EN.grad_layout(p)
    pad = torch.ones(n, dtype=torch.bool)
    for f, t in p.items():
        pad[offsets[f]:offsets[f] + t.numel()] = False
    results = []
    for fill in (0, float("nan"), 0):
        ws = torch.empty(nb // 4, dtype=torch.float32, device="cuda").fill_(fill).view(torch.uint8)
        fbuf = torch.full(((rows + 4) * E,), CANARY, device="cuda")
        feats = EN.device_forward(p, xs4, xo4, xc4, None, shape, ws, out=fbuf[:rows * E].view(S, A, E))
        assert torch.equal(fbuf[rows * E:], torch.full((4 * E,), CANARY, device="cuda")), "rows behind the features were written"
        ws = torch.empty(nb // 4, dtype=torch.float32, device="cuda").fill_(fill).view(torch.uint8)
        flat = torch.full((n + 64,), CANARY, device="cuda")
        grads, _ = EN.device_backward(p, xs4, xo4, xc4, None, shape, dy, ws, flat=flat)
        torch.cuda.synchronize()
        assert torch.equal(flat[n:], torch.full((64,), CANARY, device="cuda")), "floats behind the gradient allocation were written"
        assert bool((flat[:n][pad.cuda()] == CANARY).all()), "the padding between two gradient tensors was written"
        assert bool(torch.isfinite(flat[:n][~pad.cuda()]).all())
        results.append((feats.clone(), flat[:n].clone()))
    for feats, flat in results[1:]:
        assert torch.equal(feats, results[0][0]) and torch.equal(flat, results[0][1])
    # an env-step outside the rollout contributes nothing: its feature rows are not written, its d features (NaN here) are not read
    index = torch.tensor([4, 99, 0, -3, 20, 7], device="cuda")
    live = torch.tensor([True, False, True, False, True, True], device="cuda")
    shape_i = PT.validate("encoder", p, xs4, xo4, xc4, (), index, False)
    fbuf = torch.full((6, A, E), CANARY, device="cuda")
    EN.device_forward(p, xs4, xo4, xc4, index, shape_i, out=fbuf)
    assert bool((fbuf[~live] == CANARY).all()) and bool((fbuf[live] != CANARY).all())
    dyi = dy[:6].clone()
    dyi[~live] = float("nan")
    gi, _ = EN.device_backward(p, xs4, xo4, xc4, index, shape_i, dyi)
    gl, _ = EN.device_backward(p, xs4, xo4, xc4, index[live], PT.validate("encoder", p, xs4, xo4, xc4, (), index[live], True), dyi[live].contiguous())
    for f in gi:
        assert bool(torch.isfinite(gi[f]).all()), f
        assert torch.allclose(gi[f], gl[f], rtol=1e-4, atol=1e-5 * float(gl[f].abs().max())), f


def test_autograd_semantics():
    A, K, D, S = 3, 5, 20, 13
    _, critic = R.random_net(D, A, 811)
    obs, _ = R.random_obs(S, A, K, D, 812)
    p, xs, xo, xc = _dev(critic, obs)
    dy = torch.randn(S, A, 128, generator=torch.Generator().manual_seed(813)).cuda()
    feats, g1 = _run(p, xs, xo, xc, None, dy)
    # a parameter that does not require grad gets none; the others keep their bits
    leaves = {f: t.detach().clone().requires_grad_(f not in ("ln_w", "linear1_w")) for f, t in p.items()}
    (EN.encode(leaves, xs, xo, xc) * dy).sum().backward()
    assert leaves["ln_w"].grad is None and leaves["linear1_w"].grad is None
    assert all(torch.equal(t.grad, g1[f]) for f, t in leaves.items() if t.requires_grad)
    # two passes accumulate to exactly twice one pass
    leaves = {f: t.detach().clone().requires_grad_(True) for f, t in p.items()}
    for _ in range(2):
        (EN.encode(leaves, xs, xo, xc) * dy).sum().backward()
    assert all(torch.equal(t.grad, g1[f] + g1[f]) for f, t in leaves.items())
    # a non-contiguous incoming gradient is made contiguous
    leaves = {f: t.detach().clone().requires_grad_(True) for f, t in p.items()}
    wide = torch.zeros(S, A, 256, device="cuda")
    wide[..., ::2] = dy
    EN.encode(leaves, xs, xo, xc).backward(wide[..., ::2])
    assert all(torch.equal(t.grad, g1[f]) for f, t in leaves.items())
    # no_grad, and no parameter requiring grad: no node, the same bits
    with torch.no_grad():
        plain = EN.encode(leaves, xs, xo, xc)
    frozen = EN.encode({f: t.detach() for f, t in p.items()}, xs, xo, xc)
    assert plain.grad_fn is None and frozen.grad_fn is None and torch.equal(plain, feats) and torch.equal(frozen, feats)
    # a parameter changed in place between forward and backward: autograd's version check
    out = (EN.encode(leaves, xs, xo, xc) * dy).sum()
    with torch.no_grad():
        leaves["norm1_b"].add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.backward()
    # the module form, an optimiser of torch's own on top
    mod = EN.AttentionEncoder.from_reference({k: torch.as_tensor(v) for k, v in critic.items()}, "base.").cuda()
    assert torch.equal(mod(xs, xo, xc), feats)
    opt = torch.optim.AdamW(mod.parameters(), lr=1e-3, weight_decay=0.01)
    (mod(xs, xo, xc) * dy).sum().backward()
    assert torch.equal(mod.attn.in_proj_weight.grad, g1["in_proj_w"])
    opt.step()
    assert not torch.equal(mod(xs, xo, xc), feats)
    with pytest.raises(ValueError, match="observation gradients are not provided"):
        EN.encode(leaves, xs.clone().requires_grad_(True), xo, xc)
    with pytest.raises(ValueError, match="share one device"):
        EN.encode(leaves, xs.cpu(), xo, xc)
    with pytest.raises(IndexError, match="outside the 13 env-steps"):
        EN.encode(leaves, xs.unsqueeze(0), xo.unsqueeze(0), xc.unsqueeze(0), torch.tensor([0, 13], device="cuda"))
    with pytest.raises(ValueError, match="workspace holds"):
        EN.encode(leaves, xs, xo, xc, workspace=torch.empty(1 << 20, dtype=torch.uint8, device="cuda"))


def test_c_level_refusals_launch_nothing():
    A, K, D, S = 3, 5, 20, 9
    _, critic = R.random_net(D, A, 911)
    obs, _ = R.random_obs(S, A, K, D, 912)
    p, xs, xo, xc = _dev(critic, obs, requires_grad=False)
    xs4, xo4, xc4 = PT.as_rollout(xs, xo, xc)
    shape = PT.validate("encoder", p, xs4, xo4, xc4, (), None, True)
    lib = abi.load_library()
    rows = S * A
    nf, nb = lib.hns_encoder_workspace_bytes(rows, D, A, K, 0), lib.hns_encoder_workspace_bytes(rows, D, A, K, 1)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    feats = torch.full((rows * 128 + 4,), CANARY, device="cuda")
    dfeat = torch.ones(rows * 128 + 4, device="cuda")
    offsets, n = EN.grad_layout(p)
    flat = torch.full((n,), CANARY, device="cuda")
    grads = {f: flat[offsets[f]:offsets[f] + t.numel()] for f, t in p.items()}
    net, grd = EN._net(p), EN._net(p, grads)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def batch(**kw):
        b = PT.fill_batch(abi.HnsCriticBatch, xs4, xo4, xc4, None, shape)
        for k, v in kw.items():
            getattr(b, k)[0] = v
        return b

    def fwd(b=None, A_=A, f=feats.data_ptr(), w=nf):
        return lib.hns_encoder_forward(C.byref(net), C.byref(b if b is not None else batch()), D, A_, K, f, ws.data_ptr(), w, st)

    def bwd(b=None, A_=A, d=dfeat.data_ptr(), w=nb):
        return lib.hns_encoder_backward(C.byref(net), C.byref(b if b is not None else batch()), D, A_, K, d, C.byref(grd), ws.data_ptr(), w, st)

    cases = [(lambda: fwd(f=None), "hns_encoder_forward: null pointer"), (lambda: bwd(d=None), "hns_encoder_backward: null pointer"),
             (lambda: fwd(f=feats.data_ptr() + 4), "misaligned features"), (lambda: bwd(d=dfeat.data_ptr() + 4), "misaligned dfeatures"),
             (lambda: fwd(w=nf - 1), "workspace too small (hns_encoder_workspace_bytes)"),
             (lambda: bwd(w=nb - 1), "workspace too small (hns_encoder_workspace_bytes)"),
             (lambda: fwd(A_=0), "num_agents must be in [1, 7]"), (lambda: fwd(A_=8), "num_agents must be in [1, 7]"),
             (lambda: bwd(A_=0), "num_agents must be in [1, 7]"), (lambda: bwd(A_=8), "num_agents must be in [1, 7]"),
             (lambda: fwd(batch(self_stride=-1)), "negative stride"), (lambda: bwd(batch(cyl_stride=-1)), "negative stride")]
    for call, text in cases:
        assert call() == abi.HNS_ERR_INVALID_ARG, text
        assert text in lib.hns_last_error().decode(), (text, lib.hns_last_error().decode())
    torch.cuda.synchronize()
    assert bool((feats == CANARY).all()) and bool((flat == CANARY).all())       # nothing was launched
    # the head's fields are ignored: NULL in the parameter table and in the gradient table
    assert net.head_w is None and net.head_b is None and net.log_std is None and grd.head_w is None
    assert fwd() == abi.HNS_OK and bwd() == abi.HNS_OK
    torch.cuda.synchronize()
    assert bool((feats[:rows * 128] != CANARY).all()) and bool((feats[rows * 128:] == CANARY).all())
    assert bool(torch.isfinite(flat).all()) and bool((flat != CANARY).all())


def test_report_ratios():
    print("encoder gate ratios (worst):", {k: round(v, 2) for k, v in RATIOS.items()})
