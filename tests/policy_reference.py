"""Test-side restatement of the MAPPO actor / critic forward pass (PartialAttentionEncoder + DiagGaussian / v_out) in any float dtype.

Written out from the equations (modules/networks.py:125-163, :250-313; distributions.py:66-82), independent of hns_amd.policy: the full
attention over all N tokens (no single-query shortcut), two-pass LayerNorm, exact-erf GELU.  fp64 is the accuracy gate's yardstick, fp32 the
CPU error it is measured against."""
import math

import numpy as np
import torch

E = 128


def _ln(x, w, b):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + 1e-5) * w + b


def _lin(x, w, b):
    return x @ w.T + b


def encoder(p, prefix, obs, dtype):
    """obs: {"state_self" [.., 1, D], optional "state_others" [.., A-1, 3], "cylinders" [.., K, 5]} -> [.., 128]."""
    g = lambda n: p[prefix + n].to(dtype)
    toks = [_lin(obs[k].to(dtype), g(f"split_embed.embed.{k}.weight"), g(f"split_embed.embed.{k}.bias"))
            for k in ("state_self", "state_others", "cylinders") if k in obs]
    t = _ln(torch.cat(toks, dim=-2), g("split_embed.layer_norm.weight"), g("split_embed.layer_norm.bias"))
    W, bW = g("attn.in_proj_weight"), g("attn.in_proj_bias")
    q = _lin(t[..., :1, :], W[:E], bW[:E])
    k = _lin(t, W[E:2 * E], bW[E:2 * E])
    v = _lin(t, W[2 * E:], bW[2 * E:])
    s = (q @ k.transpose(-1, -2)) / math.sqrt(E)
    a = torch.softmax(s, dim=-1)
    attn = _lin(a @ v, g("attn.out_proj.weight"), g("attn.out_proj.bias"))
    x = _ln(t[..., :1, :] + attn, g("norm1.weight"), g("norm1.bias"))
    h = _lin(x, g("linear1.weight"), g("linear1.bias"))
    h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    y = _ln(x + _lin(h, g("linear2.weight"), g("linear2.bias")), g("norm2.weight"), g("norm2.bias"))
    return y.mean(-2)


def forward(actor, critic, obs, eps=None, dtype=torch.float64, action=None):
    """(loc, scale, action, log_prob [.., 1], value [.., 1]); `action` given: its log_prob instead of a sample's."""
    a = {k[len("module."):] if k.startswith("module.") else k: torch.as_tensor(np.asarray(v)) for k, v in actor.items()}
    c = {k[len("module."):] if k.startswith("module.") else k: torch.as_tensor(np.asarray(v)) for k, v in critic.items()}
    obs = {k: torch.as_tensor(np.asarray(v)) for k, v in obs.items()}
    y = encoder(a, "encoder.", obs, dtype)
    loc = _lin(y, a["act_dist.fc_mean.weight"].to(dtype), a["act_dist.fc_mean.bias"].to(dtype))
    scale = torch.exp(a["act_dist.log_std"].to(dtype)).expand(loc.shape)
    if action is None:
        action = loc + scale * torch.as_tensor(np.asarray(eps)).to(dtype) if eps is not None else loc
    action = torch.as_tensor(np.asarray(action)).to(dtype)
    logp = (-((action - loc) ** 2) / (2 * scale ** 2) - torch.log(scale) - math.log(math.sqrt(2 * math.pi))).sum(-1, keepdim=True)
    value = _lin(encoder(c, "base.", obs, dtype), c["v_out.weight"].to(dtype), c["v_out.bias"].to(dtype))
    return loc, scale, action, logp, value


def _bf16(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def golden_case(z, tag):
    """(actor params, critic params, obs, eps, expected dict) of one case of g_policy.npz.  Parameters are stored as bfloat16 bits, under
    "<case>:<net>:<name>" when the case has its own and "shared:<net>:<name>" otherwise (tests/golden/make_golden_policy.py)."""
    def params(which):
        out = {}
        for n in z[f"{tag}:{which}_names"]:
            key = f"{tag}:{which}:{n}"
            out[str(n)] = _bf16(z[key] if key in z.files else z[f"shared:{which}:{n}"])
        return out
    actor, critic = params("actor"), params("critic")
    obs = {k: z[f"{tag}:obs:{k}"] for k in ("state_self", "state_others", "cylinders") if f"{tag}:obs:{k}" in z.files}
    exp = {k: z[f"{tag}:{k}"] for k in ("loc", "action", "log_prob", "value", "mode")}
    return actor, critic, obs, z[f"{tag}:eps"], exp
