"""Test-side restatement of the recurrent MAPPO actor / critic forward pass (encoder -> one GRU step -> LayerNorm(h + f) -> head) in any float
dtype, and the parameter sets the recurrent policy's tests share.

Written out from the equations (modules/rnn.py:32-89 behind policy_reference.encoder), independent of hns_amd.policy and hns_amd.rnn: the gates
as separate matrix products per gate, a two-pass LayerNorm.  fp64 is the accuracy gate's yardstick, fp32 the CPU error it is measured against."""
import math

import numpy as np
import torch

import policy_reference as R

H = 128
GRU_NAMES = ("cell.weight_ih", "cell.weight_hh", "cell.bias_ih", "cell.bias_hh", "layer_norm.weight", "layer_norm.bias")
OUTPUTS = ("loc", "log_prob", "value", "actor_state", "critic_state")
BAR = R.BAR
CASES = ("a3k5d35", "a1k5d20")                              # g_policy_rnn.npz's cases: g_policy.npz's networks of the same tags


def golden_params(gp, gg, tag):
    """(actor, critic) in the reference's names for a case of g_policy_rnn.npz: encoder and head from g_policy.npz's case `tag`, the actor's GRU
    g_gru.npz's parameters, the critic's the same tensors with weight_ih <-> weight_hh and bias_ih <-> bias_hh exchanged (so that the two
    networks' GRUs differ and a swap of them shows)."""
    actor, critic, _, _, _ = R.golden_case(gp, tag)
    swap = {"cell.weight_ih": "cell.weight_hh", "cell.weight_hh": "cell.weight_ih", "cell.bias_ih": "cell.bias_hh", "cell.bias_hh": "cell.bias_ih"}
    for n in GRU_NAMES:
        actor["rnn." + n] = np.asarray(gg["param:" + n], np.float32)
        critic["rnn." + n] = np.asarray(gg["param:" + swap.get(n, n)], np.float32)
    return actor, critic


def golden_case(z, tag):
    """{name: array} of one case of g_policy_rnn.npz: obs:<key> [T, E, A, ..], eps [T, E, A, 4], is_init [T, E], h0:actor / h0:critic
    [E, A, 128], and per step loc, action, log_prob, value, actor_state, critic_state."""
    pre = tag + ":"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def step_obs(case, t):
    return {k[len("obs:"):]: v[t] for k, v in case.items() if k.startswith("obs:")}


def _gru(p, prefix, f, h, is_init, dtype):
    g = lambda n: torch.as_tensor(np.asarray(p[prefix + n])).to(dtype)
    Wi, Wh, bi, bh = g("cell.weight_ih"), g("cell.weight_hh"), g("cell.bias_ih"), g("cell.bias_hh")
    if is_init is not None:
        h = h * (1 - torch.as_tensor(np.asarray(is_init)).to(dtype).reshape(-1, 1, 1))       # env-level: all of the env's agents
    gate = lambda W, b, x, k: x @ W[k * H:(k + 1) * H].T + b[k * H:(k + 1) * H]
    r = torch.sigmoid(gate(Wi, bi, f, 0) + gate(Wh, bh, h, 0))
    z = torch.sigmoid(gate(Wi, bi, f, 1) + gate(Wh, bh, h, 1))
    n = torch.tanh(gate(Wi, bi, f, 2) + r * gate(Wh, bh, h, 2))
    h = (1 - z) * n + z * h
    return R._ln(h + f, g("layer_norm.weight"), g("layer_norm.bias")), h


def forward(actor, critic, obs, actor_state, critic_state, is_init, eps=None, dtype=torch.float64):
    """{loc, log_prob [.., 1], value [.., 1], actor_state, critic_state, action} of one step; states [E, A, 128] (None: zeros), is_init [E]
    or None."""
    a = {k[len("module."):] if k.startswith("module.") else k: torch.as_tensor(np.asarray(v)) for k, v in actor.items()}
    c = {k[len("module."):] if k.startswith("module.") else k: torch.as_tensor(np.asarray(v)) for k, v in critic.items()}
    obs = {k: torch.as_tensor(np.asarray(v)) for k, v in obs.items()}
    fa, fc = R.encoder(a, "encoder.", obs, dtype), R.encoder(c, "base.", obs, dtype)
    zero = torch.zeros(fa.shape, dtype=dtype)
    ha = torch.as_tensor(np.asarray(actor_state)).to(dtype) if actor_state is not None else zero
    hc = torch.as_tensor(np.asarray(critic_state)).to(dtype) if critic_state is not None else zero
    ya, ha = _gru(a, "rnn.", fa, ha, is_init, dtype)
    yc, hc = _gru(c, "rnn.", fc, hc, is_init, dtype)
    loc = R._lin(ya, a["act_dist.fc_mean.weight"].to(dtype), a["act_dist.fc_mean.bias"].to(dtype))
    scale = torch.exp(a["act_dist.log_std"].to(dtype)).expand(loc.shape)
    action = loc + scale * torch.as_tensor(np.asarray(eps)).to(dtype) if eps is not None else loc
    logp = (-((action - loc) ** 2) / (2 * scale ** 2) - torch.log(scale) - math.log(math.sqrt(2 * math.pi))).sum(-1, keepdim=True)
    value = R._lin(yc, c["v_out.weight"].to(dtype), c["v_out.bias"].to(dtype))
    return {"loc": loc, "log_prob": logp, "value": value, "actor_state": ha, "critic_state": hc, "action": action}


def gate_ratios(got, ref64, ref32):
    """Per output of OUTPUTS, e_got / max(e_32, 2^-24 max|ref_64|), errors as max-abs against ref64 (the rule of policy_reference)."""
    out = {}
    for name in OUTPUTS:
        h, a, b = (np.asarray(x[name], np.float64) for x in (got, ref64, ref32))
        assert h.shape == a.shape == b.shape, (name, h.shape, a.shape)
        assert np.isfinite(h).all(), f"{name}: not finite"
        e_got, e_32 = float(np.abs(h - a).max()), float(np.abs(b - a).max())
        out[name] = e_got / max(e_32, 2.0 ** -24 * float(np.abs(a).max()))
    return out


def random_net(D, A, seed):
    """policy_reference.random_net with a GRU block in each network: orthogonal weights, uniform biases and a LayerNorm affine perturbed by 0.1 N(0, 1)."""
    from hns_amd import policy as P
    actor, critic = R.random_net(D, A, seed)
    g = torch.Generator().manual_seed(seed + 13)
    for k, p in enumerate((actor, critic)):
        for n, v in P.random_rnn_parameters(seed + 100 + k).items():
            if "weight_" not in n:
                v = v + 0.1 * torch.randn(v.shape, generator=g)
            p[n] = v.numpy()
    return actor, critic


def random_states(E, A, seed):
    g = np.random.default_rng(seed)
    return (0.5 * g.standard_normal((E, A, H))).astype(np.float32), (0.5 * g.standard_normal((E, A, H))).astype(np.float32)
