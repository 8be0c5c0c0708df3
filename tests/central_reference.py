"""Test-side restatement of the centralised critic (critic_input: state; make_critic(centralized=True), learning/mappo.py:553-566, :644-660) in
any float dtype: its forward pass and MAPPOPolicy.update_critic (mappo.py:326-352) on it.

Written out from the equations on top of tests/policy_reference.py's helpers (the full attention over all tokens, two-pass LayerNorm, exact-erf
GELU) and independent of hns_amd: the encoder over the STATE spec — the A rows of state_drones through ONE Linear(D, 128), then the K cylinder
rows through Linear(5, 128), one LayerNorm over every token, token 0 (drone 0) the query — then v_out = Linear(128, A), unflattened to
[B, A, 1].  The gradients are torch autograd's.  fp64 is the accuracy gate's yardstick, fp32 the CPU error it is measured against; the rule is
the project's (policy_reference.gate_ratios, rnn_update_reference.gate): e / max(e_32, 2^-24 max|ref_64|) <= 8 per output and per gradient."""
import math

import numpy as np
import torch

import policy_reference as R
from critic_update_reference import huber

BAR = R.BAR


def _t(x):
    return torch.as_tensor(np.asarray(x))


def _params(critic):
    return {(k[len("module."):] if k.startswith("module.") else k): (v if torch.is_tensor(v) else _t(v)) for k, v in critic.items()}


def features(p, state_drones, cylinders, dtype):
    """[B, 128]: policy_reference.encoder over the state's two keys in spec order — its `state_self` slot holds the state_drones embedding
    and ALL A rows (it embeds whatever rows the key has), so the tokens are drones 0 .. A - 1, then the cylinders; the query is token 0."""
    q = {k.replace("embed.state_drones.", "embed.state_self."): v for k, v in p.items()}
    return R.encoder(q, "base.", {"state_self": state_drones, "cylinders": cylinders}, dtype)


def value(critic, state_drones, cylinders, dtype=torch.float64):
    """value [B, A, 1] as a torch tensor of `dtype` (critic: {reference name: array or tensor}; state_drones [B, A, D]; cylinders [B, K, 5])."""
    p = _params(critic)
    y = features(p, _t(state_drones), _t(cylinders), dtype)
    return R._lin(y, p["v_out.weight"].to(dtype), p["v_out.bias"].to(dtype)).unsqueeze(-1)


def value_np(critic, state_drones, cylinders, dtype=torch.float64):
    with torch.no_grad():
        return value(critic, state_drones, cylinders, dtype).double().numpy()


def loss_and_grad(critic, state_drones, cylinders, b_values, b_returns, index=None, clip_param=0.1, loss="huber", huber_delta=10.0,
                  dtype=torch.float64):
    """update_critic's statements on the minibatch `index` (env-steps; None: all) of state_drones [S, A, D], cylinders [S, K, 5], b_values and
    b_returns [S, A, 1]: critic_update_reference.loss_and_grad's dict — value_loss, l_orig, l_clip, explained_var, grad_norm (floats), branch
    (0: the unclipped loss is the larger, 1: the clipped one, 2: a tie), values and grads {name: float64 numpy}."""
    p = {k: v.to(dtype).requires_grad_(True) for k, v in _params(critic).items()}
    idx = _t(index) if index is not None else slice(None)
    sd, cyl = _t(state_drones)[idx], _t(cylinders)[idx]
    bv, ret = _t(b_values).to(dtype)[idx], _t(b_returns).to(dtype)[idx]
    fn = (lambda x: huber(x, huber_delta)) if loss == "huber" else (lambda x: x * x)
    values = R._lin(features(p, sd, cyl, dtype), p["v_out.weight"], p["v_out.bias"]).unsqueeze(-1)
    assert values.shape == bv.shape == ret.shape, (values.shape, bv.shape, ret.shape)
    clipped = bv + (values - bv).clamp(-clip_param, clip_param)
    l_clip, l_orig = fn(ret - clipped).mean(), fn(ret - values).mean()
    value_loss = torch.max(l_orig, l_clip)
    names = list(p)
    grads = torch.autograd.grad(value_loss, [p[n] for n in names])
    with torch.no_grad():
        ev = 1 - ((values - ret) ** 2).mean() / ret.var()
        norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads))
    lo, lc = float(l_orig.detach()), float(l_clip.detach())
    return {"value_loss": float(value_loss.detach()), "l_orig": lo, "l_clip": lc, "explained_var": float(ev), "grad_norm": float(norm),
            "branch": 0 if lo > lc else (1 if lo < lc else 2), "values": values.detach().double().numpy(),
            "grads": {n: g.double().numpy() for n, g in zip(names, grads)}}


def ratio(got, ref64, ref32):
    """The gate's e_got / max(e_32, 2^-24 max|ref_64|) of one output or gradient tensor; `got` must be finite and of the reference's shape."""
    h, a, b = (np.asarray(x, np.float64) for x in (got, ref64, ref32))
    assert h.shape == a.shape == b.shape, (h.shape, a.shape, b.shape)
    assert np.isfinite(h).all(), "not finite"
    e_got, e_32 = float(np.abs(h - a).max()), float(np.abs(b - a).max())
    bound = max(e_32, 2.0 ** -24 * float(np.abs(a).max()))
    return e_got / bound if bound > 0 else (0.0 if e_got == 0 else math.inf)


def gate_update(tag, got, r64, r32, log=print):
    """Every scalar, `values` and every gradient of `got` (loss_and_grad's dict layout) against the fp64 / fp32 restatements under the rule;
    returns the worst ratio, raises AssertionError naming every tensor over the bar."""
    worst, bad = 0.0, []
    items = [(n, got[n], r64[n], r32[n]) for n in ("value_loss", "explained_var", "grad_norm", "values")]
    items += [(n, got["grads"][n], r64["grads"][n], r32["grads"][n]) for n in r64["grads"]]
    for name, h, a, b in items:
        x = ratio(h, a, b)
        log(f"  {tag} {name}: ratio {x:.2f}")
        worst = max(worst, x)
        if not x <= BAR:
            bad.append(f"{name}: ratio {x:.2f}")
    assert not bad, f"{tag}: " + "; ".join(bad)
    return worst


def golden_case(z, tag):
    """(critic {name: fp32 array}, state_drones, cylinders, expected value) of one case of g_policy_central.npz (parameters as bfloat16 bits under
    "<case>:critic:<name>" when the case has its own and "shared:critic:<name>" otherwise; tests/golden/make_golden_policy_central.py)."""
    critic = {}
    for n in z[f"{tag}:critic_names"]:
        key = f"{tag}:critic:{n}"
        critic[str(n)] = R._bf16(z[key] if key in z.files else z[f"shared:critic:{n}"])
    return critic, z[f"{tag}:state_drones"], z[f"{tag}:cylinders"], z[f"{tag}:value"]


def random_critic(D, A, seed, head_scale=30.0):
    """hns_amd.policy.random_parameters_central's critic with every bias and norm perturbed and v_out scaled so that values are of order 0.3
    (the clip at 0.1 cuts some values and not others), as numpy fp32 in registration order."""
    from hns_amd import policy as P
    _, critic = P.random_parameters_central(D, A, seed)
    g = torch.Generator().manual_seed(seed + 7)
    for k, v in critic.items():
        if k.endswith("bias") or "norm" in k:
            critic[k] = v + torch.randn(v.shape, generator=g) * 0.1
        if k == "v_out.weight":
            critic[k] = v * head_scale
    return {k: v.numpy().astype(np.float32) for k, v in critic.items()}


def random_state(S, A, K, D, seed):
    """(state_drones [S, A, D], cylinders [S, K, 5]) with some zero (inactive) cylinder rows."""
    g = np.random.default_rng(seed)
    sd = (g.standard_normal((S, A, D)) * 0.7).astype(np.float32)
    cyl = (g.standard_normal((S, K, 5)) * 0.5).astype(np.float32)
    cyl[g.random((S, K)) < 0.2] = 0.0
    return sd, cyl


def targets(critic, sd, cyl, seed, ret_scale=1.0, bv_noise=0.1, shift=None):
    """test_hip_critic_train._targets for the centralised critic: b_values near the critic's own values, returns around them; `shift`: half
    of the values get old values |shift| nearer to (+) or further from (-) the returns, which decides the branch of the max."""
    v = value_np(critic, sd, cyl, torch.float32)
    g = np.random.default_rng(seed)
    bv = (v + g.standard_normal(v.shape) * bv_noise).astype(np.float32)
    ret = ((v + g.standard_normal(v.shape)) * ret_scale).astype(np.float32)
    if shift is not None:
        half = g.random(v.shape) < 0.5
        bv = np.where(half, v + shift * np.sign(ret - v), v + (bv - v) * 0.3).astype(np.float32)
    return bv, ret
