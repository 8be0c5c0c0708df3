"""Test-side restatement of MAPPOPolicy.update_critic (learning/mappo.py:326-352) in any float dtype, on top of tests/policy_reference.py (the
full attention over all tokens, written out from the equations, independent of hns_amd): value loss, explained variance, the gradients by
torch autograd, clip_grad_norm_ and Adam.  fp64 autograd is the accuracy gate's yardstick, fp32 the CPU error it is measured against.
`clip_np` / `clip_adam_np` restate clip_grad_norm_'s scaling and torch.optim.Adam's single-tensor statements in numpy fp32: what
hns_adam_clipped is held to, bit for bit."""
import numpy as np
import torch

import policy_reference as R


def _strip(d):
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in d.items()}


def huber(x, delta):
    ax = x.abs()
    return torch.where(ax < delta, 0.5 * x * x, delta * (ax - 0.5 * delta))


def loss_and_grad(critic, obs, b_values, b_returns, index=None, clip_param=0.1, loss="huber", huber_delta=10.0, dtype=torch.float64, chunk=8192):
    """critic: {reference name: array}; obs: {"state_self" [S, A, 1, D], optional "state_others", "cylinders"} over S env-steps; b_values,
    b_returns [S, A, 1]; index: env-steps of the minibatch.  Returns a dict: value_loss, l_orig, l_clip, explained_var, grad_norm (floats),
    branch (0: the unclipped loss is the larger, 1: the clipped one, 2: a tie), values and grads {name: float64 numpy}.

    A minibatch of at most `chunk` env-steps is update_critic's statements as written (autograd through torch.max of the two means).  A larger
    one (the attention over all tokens in fp64 does not fit in memory) runs in chunks: the two means first, then autograd of
    (w_orig sum loss(values) + w_clip sum loss(clipped)) / n per chunk with the weights torch.max's backward gives — (1, 0), (0, 1) or halves."""
    p = {k: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in _strip(critic).items()}
    idx = torch.as_tensor(np.asarray(index)) if index is not None else None
    o = {k: (torch.as_tensor(np.asarray(v))[idx] if idx is not None else torch.as_tensor(np.asarray(v))) for k, v in obs.items()}
    bv, ret = (torch.as_tensor(np.asarray(t)).to(dtype) for t in (b_values, b_returns))
    if idx is not None:
        bv, ret = bv[idx], ret[idx]
    fn = (lambda x: huber(x, huber_delta)) if loss == "huber" else (lambda x: x * x)
    names = list(p)
    B = bv.shape[0]

    def fwd(s, e):
        values = R._lin(R.encoder(p, "base.", {k: v[s:e] for k, v in o.items()}, dtype), p["v_out.weight"], p["v_out.bias"])
        assert values.shape == bv[s:e].shape == ret[s:e].shape, (values.shape, bv.shape, ret.shape)
        return values, bv[s:e] + (values - bv[s:e]).clamp(-clip_param, clip_param)

    if B <= chunk:
        values, clipped = fwd(0, B)
        l_clip, l_orig = fn(ret - clipped).mean(), fn(ret - values).mean()
        value_loss = torch.max(l_orig, l_clip)
        grads = torch.autograd.grad(value_loss, [p[n] for n in names])
        values = values.detach()
    else:
        n = float(ret.numel())
        with torch.no_grad():
            parts = [fwd(s, min(s + chunk, B)) for s in range(0, B, chunk)]
            values = torch.cat([v for v, _ in parts])
            l_orig = sum(fn(ret[s:s + chunk] - v).sum() for s, (v, _) in zip(range(0, B, chunk), parts)) / n
            l_clip = sum(fn(ret[s:s + chunk] - c).sum() for s, (_, c) in zip(range(0, B, chunk), parts)) / n
            value_loss = torch.max(l_orig, l_clip)
        w0, w1 = (1.0, 0.0) if l_orig > l_clip else ((0.0, 1.0) if l_orig < l_clip else (0.5, 0.5))
        grads = None
        for s in range(0, B, chunk):
            v, c = fwd(s, min(s + chunk, B))
            part = (w0 * fn(ret[s:s + chunk] - v).sum() + w1 * fn(ret[s:s + chunk] - c).sum()) / n
            gs = torch.autograd.grad(part, [p[k] for k in names])
            grads = gs if grads is None else [a + b for a, b in zip(grads, gs)]
    with torch.no_grad():
        ev = 1 - ((values - ret) ** 2).mean() / ret.var()
        norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads))
    lo, lc = float(l_orig.detach()), float(l_clip.detach())
    return {"value_loss": float(value_loss.detach()), "l_orig": lo, "l_clip": lc, "explained_var": float(ev), "grad_norm": float(norm),
            "branch": 0 if lo > lc else (1 if lo < lc else 2), "values": values.detach().double().numpy(),
            "grads": {n: g.double().numpy() for n, g in zip(names, grads)}}


def golden_case(zc, zp, tag):
    """One case of g_critic_update.npz (tests/golden/make_golden_critic_update.py) with its critic parameters from g_policy.npz: (critic
    {name: fp32 array} in the module's parameter order, obs, b_values, b_returns, index, loss, recorded {key: array})."""
    _, critic, _, _, _ = R.golden_case(zp, tag)
    critic = {str(n): critic[str(n)] for n in zc[f"{tag}:names"]}
    obs = {k: zc[f"{tag}:obs:{k}"] for k in ("state_self", "state_others", "cylinders") if f"{tag}:obs:{k}" in zc.files}
    rec = {k[len(tag) + 1:]: zc[k] for k in zc.files if k.startswith(tag + ":")}
    return critic, obs, zc[f"{tag}:b_values"], zc[f"{tag}:b_returns"], zc[f"{tag}:index"], str(zc[f"{tag}:loss"]), rec


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def clip_np(grads, total_norm, max_norm):
    """clip_grad_norm_'s scaling in fp32: coef = min((1 / (norm + 1e-6)) * max_norm, 1) (torch forms max_norm / x as reciprocal(x) * max_norm),
    every gradient times coef — always, also when coef is 1."""
    f32 = np.float32
    coef = f32(f32(f32(1.0) / f32(f32(total_norm) + f32(1e-6))) * f32(max_norm))
    coef = f32(min(coef, f32(1.0)))
    return [(g * coef).astype(f32) for g in grads], coef


def adam_np(p, g, m, v, step, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, sqrt=np.sqrt):
    """torch.optim.Adam's single-tensor statements in numpy fp32 with `step` already bumped (tests/test_tp_train.py's adam_np, which bumps it
    itself): returns p, m, v.  `sqrt`: IEEE (the kernel's); torch's CPU sqrt is not correctly rounded, so a CPU self-check passes torch's in."""
    b1, b2 = betas
    f32 = np.float32
    m = _fma32(f32(1 - b1), (g - m).astype(f32), m)
    v = _fma32((f32(1 - b2) * g).astype(f32), g, (v * f32(b2)).astype(f32))
    bc1 = 1 - b1 ** float(step)
    bc2 = 1 - b2 ** float(step)
    den = (sqrt(v) / f32(bc2 ** 0.5)).astype(f32) + f32(eps)
    p = (p + (f32(-(lr / bc1)) * m).astype(f32) / den).astype(f32)
    return p, m, v


def clip_adam_np(params, grads, ms, vs, step, total_norm, max_norm, **kw):
    """One ClippedAdam step over lists of arrays: (params, clipped grads, ms, vs, step + 1)."""
    if max_norm is not None and np.isfinite(max_norm):
        grads, _ = clip_np(grads, total_norm, max_norm)
    step = np.float32(np.float32(step) + np.float32(1.0))
    out = [adam_np(p, g, m, v, step, **kw) for p, g, m, v in zip(params, grads, ms, vs)]
    return [o[0] for o in out], grads, [o[1] for o in out], [o[2] for o in out], step
