"""Shared by test_dp_learner.py and test_hip_dp_learner.py: the numpy restatement of hns_grad_norm's documented order (include/hns.h), the
accuracy bar of the update tests applied to a gradient that several ranks summed, and the inputs of the branch-flip case.

The bar is test_hip_critic_train.py's: e <= BAR max(e_32, 2^-24 max|g_64|) per tensor, errors as max-abs against fp64 autograd over the UNION
of the ranks' minibatches (tests/actor_update_reference.py, tests/critic_update_reference.py), e_32 the error of the same statements in CPU
torch fp32 autograd over the union.  BAR is imported from there, not restated."""
import math

import numpy as np
import torch

import actor_update_reference as UA
import critic_update_reference as UC
import learner_f64_reference as FR
from test_hip_critic_train import BAR, _net, _obs, _targets


def grad_norm(flat):
    """hns_grad_norm on a flat fp32 array, operation by operation: quads of four floats (the short last one padded with zeros), G =
    clamp(ceil(quads / 1024), 1, 64) workgroups of 256 threads, thread t adds quads t, t + 256 G, ... in order, per wave the butterfly over
    lane ^ 32, 16, 8, 4, 2, 1, the four waves in index order, the G partials in index order, one fp64 square root rounded once to fp32."""
    x = np.asarray(flat, np.float32).reshape(-1)
    quads = (x.size + 3) // 4
    pad = np.zeros(quads * 4, np.float64)
    pad[:x.size] = x
    q = pad.reshape(quads, 4)
    ss = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
    G = min(max(-(-quads // 1024), 1), 64)
    T = 256 * G
    acc = np.zeros(T, np.float64)
    for start in range(0, quads, T):
        part = ss[start:start + T]
        acc[:part.size] += part
    lanes = np.arange(64)
    total = 0.0
    for b in range(G):
        s = acc[b * 256:(b + 1) * 256].reshape(4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        wg = 0.0
        for w in range(4):
            wg += s[w, 0]
        total += wg
    return np.float32(np.sqrt(total))


def ulps(a, b):
    """The distance of two fp32 values of one sign in units of the last place."""
    ia, ib = (int(np.float32(v).view(np.int32)) for v in (a, b))
    return abs(ia - ib)


def ratios(items):
    """items: (name, got, ref64, ref32) -> {name: e / max(e_32, 2^-24 max|ref64|)} (inf where the bound is 0 and the error is not)."""
    out = {}
    for name, h, a, b in items:
        h, a, b = (np.asarray(v, np.float64) for v in (h, a, b))
        assert h.shape == a.shape and np.isfinite(h).all(), name
        e, e32 = float(np.abs(h - a).max()), float(np.abs(b - a).max())
        bound = max(e32, 2.0 ** -24 * float(np.abs(a).max()))
        out[name] = e / bound if bound > 0 else (0.0 if e == 0 else math.inf)
    return out


def assert_within_bar(tag, items):
    r = ratios(items)
    print(f"  {tag}: worst ratio {max(r.values()):.2f} ({max(r, key=r.get)})")
    bad = {k: round(v, 2) for k, v in r.items() if not v <= BAR}
    assert not bad, f"{tag}: beyond {BAR} x max(e_32, 2^-24 max|g_64|): {bad}"
    return r


def critic_refs(critic, obs, bv, ret, **kw):
    """fp64 and fp32 autograd over the union (critic: {reference name: array}; obs, bv, ret over the union's env-steps)."""
    return UC.loss_and_grad(critic, obs, bv, ret, None, dtype=torch.float64, **kw), UC.loss_and_grad(critic, obs, bv, ret, None, dtype=torch.float32, **kw)


def actor_refs(actor, obs, action, lpo, adv, **kw):
    return (UA.loss_and_grad(actor, obs, action, lpo, adv, None, dtype=torch.float64, **kw),
            UA.loss_and_grad(actor, obs, action, lpo, adv, None, dtype=torch.float32, **kw))


def grad_items(got, r64, r32):
    return [(k, got[k], r64["grads"][k], r32["grads"][k]) for k in r64["grads"]]


def branch_flip_case(A=3, K=5, D=20, steps=(7, 4), seed=941):
    """The construction of tests/golden/make_golden_critic_update.py (test_hip_critic_train._targets' `shift`): half of the rows get old
    values |shift| nearer to (+) or further from (-) the returns than the new ones.  Rank 0's env-steps are shifted TOWARD the returns by 0.3
    (alone: the unclipped mean is the larger, branch 0), rank 1's AWAY by 0.9 (the clipped mean is the larger, branch 1, and by enough to
    decide the union).  Returns (critic, obs, bv, ret, slices) over the union's env-steps, rank r owning slices[r]."""
    critic = _net(D, A, seed)
    S = sum(steps)
    obs = _obs(S, A, K, D, seed + 1)
    sl = [slice(0, steps[0]), slice(steps[0], S)]
    parts = [_targets(critic, {k: v[s] for k, v in obs.items()}, seed + 2 + r, shift=sh) for r, (s, sh) in enumerate(zip(sl, (0.3, -0.9)))]
    bv, ret = (np.concatenate([p[i] for p in parts]) for i in (0, 1))
    return critic, obs, bv, ret, sl


def assert_branch_precondition(critic, obs, bv, ret, sl, **kw):
    """Rank 0 alone takes the unclipped branch, rank 1 alone and the union the clipped one, each pair of means >= 1e-3 of the loss apart (fp64)."""
    seen = []
    for s in (*sl, slice(None)):
        r = UC.loss_and_grad(critic, {k: v[s] for k, v in obs.items()}, bv[s], ret[s], None, dtype=torch.float64, **kw)
        assert abs(r["l_orig"] - r["l_clip"]) >= 1e-3 * r["value_loss"], (s, r["l_orig"], r["l_clip"])
        seen.append(r["branch"])
    assert seen == [0, 1, 1], seen


obs_dict = FR.obs_dict
