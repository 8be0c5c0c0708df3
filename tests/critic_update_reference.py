"""Test-side restatement of MAPPOPolicy.update_critic (learning/mappo.py:326-352) in any float dtype, on top of tests/policy_reference.py (the
full attention over all tokens, written out from the equations, independent of hns_amd): value loss, explained variance, the gradients by
torch autograd, clip_grad_norm_ and Adam.  fp64 autograd is the accuracy gate's yardstick, fp32 the CPU error it is measured against.
`clip_np` / `adam_np` / `clip_adam_np`, the numpy fp32 restatement hns_adam_clipped is held to bit for bit, are tests/adam_reference.py's, re-exported."""
import numpy as np
import torch

import policy_reference as R
from adam_reference import adam_np, clip_adam_np, clip_np  # noqa: F401


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
