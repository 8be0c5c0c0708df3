"""Test-side restatement of the recurrent MAPPO actor / critic forward pass (encoder -> one GRU step -> LayerNorm(h + f) -> head) in any float
dtype, and the parameter sets the recurrent policy's tests share.

Written out from the equations (modules/rnn.py:32-89 behind policy_reference.encoder), independent of hns_amd.policy and hns_amd.rnn: the gates
as separate matrix products per gate, a two-pass LayerNorm.  fp64 is the accuracy gate's yardstick, fp32 the CPU error it is measured against.

Below it `emulate_step`, the recurrent kernels' ALGORITHM in fp32 (tiles of 32 rows, the flag's env index, the masked state, the gate order of
pol_gru_step) with thirteen seedable defects (`DEFECTS`): the teeth of the gate, tests/test_policy_rnn.py.  The cases are policy_rnn_cases.py's."""
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


def add_random_gru(actor, critic, seed):
    """A GRU block into each network's dict (in place; returns both): orthogonal weights, uniform biases and a LayerNorm affine perturbed by
    0.1 N(0, 1)."""
    from hns_amd import policy as P
    g = torch.Generator().manual_seed(seed + 13)
    for k, p in enumerate((actor, critic)):
        for n, v in P.random_rnn_parameters(seed + 100 + k).items():
            if "weight_" not in n:
                v = v + 0.1 * torch.randn(v.shape, generator=g)
            p[n] = v.numpy()
    return actor, critic


def random_net(D, A, seed):
    """policy_reference.random_net with a GRU block in each network (add_random_gru)."""
    return add_random_gru(*R.random_net(D, A, seed), seed)


def random_states(E, A, seed):
    g = np.random.default_rng(seed)
    return (0.5 * g.standard_normal((E, A, H))).astype(np.float32), (0.5 * g.standard_normal((E, A, H))).astype(np.float32)


def mode_log_prob(actor, shape, dtype):
    """log_prob [*shape, 1] at the mode (action = loc): `forward`'s sum with its first term zero, in `dtype`."""
    scale = torch.exp(torch.as_tensor(np.asarray(actor["act_dist.log_std"])).to(dtype))
    return (-torch.log(scale) - math.log(math.sqrt(2 * math.pi))).sum(-1, keepdim=True).expand(*shape, 1).clone()


# ---------------------------------------------------------------------------------------------------------------------------------------
# The recurrent kernels' algorithm (csrc/hns_policy.hip: pol_gru_step behind pol_encoder) in fp32: not autograd, not `forward` at a dtype.
# It keeps what the kernel decides — rows in tiles of 32 with row0 = 32 tile, the flag of row row0 + r read at env (row0 + r) / A, a zero
# state for flagged rows, rows past the end and a NULL state (selected, never multiplied: a flagged row's h_in is not read), b_ir + b_hr and
# b_iz + b_hz rounded once, each gate from its bias with the x product before the h product, 1 / (1 + exp(-a)), b_hn inside r,
# h' = (1 - z) n + z h, LayerNorm(h' + f) with eps 1e-5 and the biased variance, the critic on the second half of the GRU image — and not the
# MFMA's rounding order inside a product.  The encoder features are policy_reference's emulation.
TILE = 32
DEFECTS = ("flag_env_split_division", "flag_by_row", "hh_rz_swapped", "bhh_rz_dropped", "bhn_outside_r", "blend_with_unmasked_h",
           "mask_after_cell", "norm_of_old_state", "norm_eps_0", "norm_unbiased_variance", "critic_flags_ignored",
           "critic_norm_affine_from_actor", "critic_hh_from_actor_state")


def _sigm(a):
    return 1.0 / (1.0 + torch.exp(-a))


def _emulate_gru(p, f, h, keep, defect, ln=None, h_prod=None):
    """(LayerNorm(h' + f), h') of one network's rows [R, 128].  h: the caller's state, read where `keep` [R, 1] holds; ln: the (weight, bias)
    the norm uses if not the network's own; h_prod: the masked state the h products read if not the network's own."""
    g = lambda n: p["rnn." + n]
    Wi, Wh, bi, bh = g("cell.weight_ih"), g("cell.weight_hh"), g("cell.bias_ih"), g("cell.bias_hh")
    hm = torch.where(keep, h, torch.zeros_like(h))
    hp = h if defect == "mask_after_cell" else hm                # the state the cell sees
    hx = hp if h_prod is None else h_prod                        # ... and the one its three h products read
    b_r, b_z = (bi[:H], bi[H:2 * H]) if defect == "bhh_rz_dropped" else (bi[:H] + bh[:H], bi[H:2 * H] + bh[H:2 * H])
    W_hr, W_hz = (Wh[H:2 * H], Wh[:H]) if defect == "hh_rz_swapped" else (Wh[:H], Wh[H:2 * H])
    r = _sigm((b_r + f @ Wi[:H].T) + hx @ W_hr.T)
    if defect == "bhn_outside_r":
        rn = r * (hx @ Wh[2 * H:].T) + bh[2 * H:]
    else:
        rn = r * (bh[2 * H:] + hx @ Wh[2 * H:].T)
    n = torch.tanh((bi[2 * H:] + f @ Wi[2 * H:].T) + rn)
    z = _sigm((b_z + f @ Wi[H:2 * H].T) + hx @ W_hz.T)
    hn = (1.0 - z) * n + z * (h if defect == "blend_with_unmasked_h" else hp)
    if defect == "mask_after_cell":
        hn = torch.where(keep, hn, torch.zeros_like(hn))
    w, b = ln if ln is not None else (g("layer_norm.weight"), g("layer_norm.bias"))
    y = (hm if defect == "norm_of_old_state" else hn) + f
    y = y - y.sum(-1, keepdim=True) * (1.0 / H)
    var = (y * y).sum(-1, keepdim=True) * (1.0 / (H - 1) if defect == "norm_unbiased_variance" else 1.0 / H)
    rstd = 1.0 / torch.sqrt(var + (0.0 if defect == "norm_eps_0" else 1e-5))
    return (y * rstd) * w + b, hn


def emulate_step(actor, critic, obs, actor_state, critic_state, is_init, eps, defect=None, features=None):
    """{loc, log_prob [.., 1], value [.., 1], actor_state, critic_state, action} of one step as fp32 numpy, by the kernel's algorithm (above).
    States [E, A, 128] or None (a NULL state), is_init [E] or None, eps None: the mode.  `defect` seeds one subtle error (DEFECTS).
    features: policy_reference.emulate_features(actor, critic, obs) if the caller has them already (they do not depend on the defect)."""
    assert defect is None or defect in DEFECTS, defect
    f32 = torch.float32
    a, c = R._f32_params(actor), R._f32_params(critic)
    fa, fc = features if features is not None else R.emulate_features(actor, critic, obs)
    E_, A = fa.shape[:2]
    rows = E_ * A
    with torch.no_grad():
        row = torch.arange(rows)
        row0 = row // TILE * TILE                                # the row's tile starts at row0; the row is its r-th
        r = row - row0
        flagged = torch.zeros(rows, dtype=torch.bool)
        if is_init is not None:
            flags = torch.as_tensor(np.asarray(is_init)).reshape(E_) != 0
            if defect == "flag_env_split_division":
                flagged = flags[row0 // A + r // A]
            elif defect == "flag_by_row":
                flagged = torch.where(row < E_, flags[row.clamp(max=E_ - 1)], torch.zeros(rows, dtype=torch.bool))  # (past the flags: unset)
            else:
                flagged = flags[(row0 + r) // A]
        state = lambda h: torch.as_tensor(np.asarray(h)).to(f32).reshape(rows, H) if h is not None else None
        ha, hc = state(actor_state), state(critic_state)
        keep = lambda h, fl: (~fl).reshape(rows, 1) if h is not None else torch.zeros(rows, 1, dtype=torch.bool)
        zero = torch.zeros(rows, H)
        fa, fc = fa.reshape(rows, H), fc.reshape(rows, H)
        keep_a = keep(ha, flagged)
        ya, na = _emulate_gru(a, fa, ha if ha is not None else zero, keep_a, defect)
        keep_c = keep(hc, torch.zeros_like(flagged) if defect == "critic_flags_ignored" else flagged)
        ln = (a["rnn.layer_norm.weight"], a["rnn.layer_norm.bias"]) if defect == "critic_norm_affine_from_actor" else None
        stale = torch.where(keep_a, ha if ha is not None else zero, zero) if defect == "critic_hh_from_actor_state" else None
        yc, nc = _emulate_gru(c, fc, hc if hc is not None else zero, keep_c, defect, ln=ln, h_prod=stale)
        loc, lp = R.emulate_head(a, ya.reshape(E_, A, H), eps)
        action = loc + torch.exp(a["act_dist.log_std"]) * torch.as_tensor(np.asarray(eps)).to(f32) if eps is not None else loc
        value = yc.reshape(E_, A, H) @ c["v_out.weight"].T + c["v_out.bias"]
    out = {"loc": loc, "log_prob": lp, "value": value, "actor_state": na.reshape(E_, A, H), "critic_state": nc.reshape(E_, A, H), "action": action}
    return {k: v.numpy() for k, v in out.items()}
