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


# ---------------------------------------------------------------------------------------------------------------------------------------
# The accuracy rule of the policy tests, and the committed cases it is applied to on the CPU (test_policy_net.py: an fp32 emulation of the
# kernel's algorithm, with and without seeded defects) and on the GPU (test_hip_policy.py, test_hip_policy_edges.py: the kernel itself).
BAR = 8.0
OUTPUTS = ("loc", "log_prob", "value")


def gate_ratios(got, ref64, ref32):
    """Per output, e_got / max(e_32, 2^-24 max|ref_64|) with errors as max-abs against ref64; every `got` value must be finite."""
    out = {}
    for name, h, a, b in zip(OUTPUTS, got, ref64, ref32):
        h, a, b = (np.asarray(x, np.float64) for x in (h, a, b))
        assert h.shape == a.shape == b.shape, (name, h.shape, a.shape)
        assert np.isfinite(h).all(), f"{name}: not finite"
        e_got, e_32 = float(np.abs(h - a).max()), float(np.abs(b - a).max())
        out[name] = e_got / max(e_32, 2.0 ** -24 * float(np.abs(a).max()))
    return out


def reference_outputs(actor, critic, obs, eps, dtype, chunk=8192):
    """[loc, log_prob, value] of the restatement as fp64 numpy, in chunks of envs (the full attention in fp64 is memory-hungry)."""
    n = obs["state_self"].shape[0]
    outs = []
    for s in range(0, n, chunk):
        o = {k: v[s:s + chunk] for k, v in obs.items()}
        loc, _, _, logp, value = forward(actor, critic, o, eps[s:s + chunk] if eps is not None else None, dtype=dtype)
        outs.append((loc.double().numpy(), logp.double().numpy(), value.double().numpy()))
    return [np.concatenate([o[i] for o in outs]) for i in range(3)]


def random_net(D, A, seed, weight_scale=1.0, embed_scale=1.0, log_std=None):
    """hns_amd.policy.random_parameters with every bias, norm and log_std perturbed (the initialisers leave most of them 0 or 1)."""
    from hns_amd import policy as P
    actor, critic = P.random_parameters(D, A, seed)
    g = torch.Generator().manual_seed(seed + 7)
    for p in (actor, critic):
        for k, v in p.items():
            if k.endswith("bias") or "norm" in k or "log_std" in k:
                p[k] = v + torch.randn(v.shape, generator=g) * 0.1
            if "in_proj_weight" in k:
                p[k] = p[k] * weight_scale
            if "split_embed.embed" in k and k.endswith("weight"):
                p[k] = p[k] * embed_scale
    if log_std is not None:
        actor["act_dist.log_std"] = torch.tensor(log_std, dtype=torch.float32)
    return {k: v.numpy() for k, v in actor.items()}, {k: v.numpy() for k, v in critic.items()}


def random_obs(E_, A, K, D, seed, scale=1.0):
    g = np.random.default_rng(seed)
    obs = {"state_self": (g.standard_normal((E_, A, 1, D)) * 0.7 * scale).astype(np.float32)}
    if A > 1:
        obs["state_others"] = (g.standard_normal((E_, A, A - 1, 3)) * 0.5 * scale).astype(np.float32)
    obs["cylinders"] = (g.standard_normal((E_, A, K, 5)) * 0.5 * scale).astype(np.float32)
    return obs, g.standard_normal((E_, A, 4)).astype(np.float32)


EDGES = ("flat_tokens", "saturated_softmax", "large_obs")


def edge_case(mode):
    """The three numerical edges: near-constant tokens (LayerNorm variance ~ 0), a saturated softmax, observations of magnitude ~300."""
    if mode == "flat_tokens":
        actor, critic = random_net(20, 3, 21, embed_scale=1e-4)
        for p in (actor, critic):
            for k in p:
                if "split_embed.embed" in k and k.endswith("bias"):
                    p[k] = (np.full_like(p[k], 0.3) + np.linspace(0, 1e-3, p[k].size, dtype=np.float32)).astype(np.float32)
    elif mode == "saturated_softmax":
        actor, critic = random_net(20, 3, 22, weight_scale=40.0)
    else:
        actor, critic = random_net(20, 3, 23)
    obs, eps = random_obs(1024, 3, 8, 20, 24, scale=300.0 if mode == "large_obs" else 1.0)
    return actor, critic, obs, eps


# (A, K, D, E): one value at its limit per case, the others ordinary.  A = 1, 2 (exactly one state_others token) and 7; K = 1 and 16; D = 1
# and 96 (HNS_POLICY_MAX_SELF_DIM); E A = 1, 31, 32 and 33 rows around the kernel's 32-row tile; E = 1 with three agents.
LIMIT_SHAPES = [(1, 5, 20, 40), (2, 5, 20, 40), (7, 5, 20, 9), (3, 1, 20, 33), (3, 16, 20, 33), (3, 5, 1, 33), (3, 5, 96, 33),
                (1, 5, 35, 1), (1, 5, 35, 31), (4, 5, 35, 8), (3, 5, 35, 11), (3, 5, 35, 1)]


def limit_tag(shape):
    return "limit-a%dk%dd%de%d" % tuple(shape)


def limit_case(shape):
    A, K, D, E_ = shape
    seed = 500 + 1000 * A + 100 * K + D + 7 * E_
    actor, critic = random_net(D, A, seed)
    obs, eps = random_obs(E_, A, K, D, seed + 1)
    return actor, critic, obs, eps


LOG_STD = [-0.5, 0.2, 0.6, -0.1]


def log_std_case():
    """A log_std that differs per component (test_hip_actor_train.py's values): a kernel that reads one component's for all four fails."""
    actor, critic = random_net(35, 3, 41, log_std=LOG_STD)
    obs, eps = random_obs(203, 3, 5, 35, 42)
    return actor, critic, obs, eps


def _f32_params(params):
    return {k[len("module."):] if k.startswith("module.") else k: torch.as_tensor(np.asarray(v)).to(torch.float32) for k, v in params.items()}


def _emulate_ln(x, w, b, ln_eps=1e-5):
    x = x - x.sum(-1, keepdim=True) * (1.0 / E)
    rstd = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) * (1.0 / E) + ln_eps)
    return (x * rstd) * w + b


def _emulate_encoder(p, prefix, obs, defect=None):
    """One network's features [.., 128] by the kernel's algorithm (emulate_kernel's docstring) in fp32; p and obs hold fp32 tensors."""
    f32 = torch.float32
    ln_eps = 0.0 if defect == "layernorm_eps_0" else 1e-5
    ln = lambda x, w, b: _emulate_ln(x, w, b, ln_eps)
    g = lambda n: p[prefix + n]
    lnw, lnb = g("split_embed.layer_norm.weight"), g("split_embed.layer_norm.bias")
    tok = lambda key, bias_key: ln(obs[key] @ g(f"split_embed.embed.{key}.weight").T + g(f"split_embed.embed.{bias_key}.bias"), lnw, lnb)
    toks = [tok("state_self", "state_self")]
    if "state_others" in obs:
        toks.append(tok("state_others", "cylinders" if defect == "others_with_cylinder_bias" else "state_others"))
    toks.append(tok("cylinders", "cylinders"))
    t = torch.cat(toks, dim=-2)
    if defect == "last_cylinder_skipped":
        t = t[..., :-1, :]
    t0 = t[..., 0, :]
    W, bW = g("attn.in_proj_weight"), g("attn.in_proj_bias")
    q = t0 @ W[:E].T + bW[:E]
    rs = torch.tensor(1.0 / math.sqrt(E), dtype=f32)
    if defect == "score_scale_bf16":
        rs = rs.to(torch.bfloat16).to(f32)
    kq = (q @ W[E:2 * E]) * rs                               # W_k^T q / sqrt(128)
    s = (t * kq.unsqueeze(-2)).sum(-1)
    m, l, z = s[..., 0], torch.ones_like(s[..., 0]), t0.clone()
    for j in range(1, t.shape[-2]):
        mn = torch.maximum(s[..., j], m)
        cj, pj = torch.exp(m - mn), torch.exp(s[..., j] - mn)
        l = l * cj + pj
        z = pj.unsqueeze(-1) * t[..., j, :] + (z if defect == "softmax_rescale_omitted" else z * cj.unsqueeze(-1))
        m = mn
    z = z * (1.0 / l).unsqueeze(-1)
    v = z @ W[2 * E:].T
    if defect != "value_bias_dropped":
        v = v + bW[2 * E:]
    attn = v @ g("attn.out_proj.weight").T + g("attn.out_proj.bias")
    x = ln(t0 + attn, g("norm1.weight"), g("norm1.bias"))
    h = x @ g("linear1.weight").T + g("linear1.bias")
    if defect == "gelu_tanh":
        h = 0.5 * h * (1.0 + torch.tanh(0.7978845608028654 * (h + 0.044715 * h * h * h)))
    else:
        h = 0.5 * h * (1.0 + torch.erf(h * 0.7071067811865476))
    return ln(x + (h @ g("linear2.weight").T + g("linear2.bias")), g("norm2.weight"), g("norm2.bias"))


def emulate_features(actor, critic, obs):
    """(actor features, critic features) [E, A, 128] as fp32 tensors: what emulate_kernel's two encoder passes hand to the heads (and the
    recurrent step's emulation, policy_rnn_reference.emulate_step, to its GRUs)."""
    a, c = _f32_params(actor), _f32_params(critic)
    obs = {k: torch.as_tensor(np.asarray(v)).to(torch.float32) for k, v in obs.items()}
    with torch.no_grad():
        return _emulate_encoder(a, "encoder.", obs), _emulate_encoder(c, "base.", obs)


def emulate_head(a, y, eps, defect=None):
    """(loc, log_prob [.., 1]) of the kernel's DiagGaussian head on the actor's features y (fp32 tensors): the log-probability summed in
    component order.  eps None: the mode."""
    f32 = torch.float32
    loc = y @ a["act_dist.fc_mean.weight"].T + a["act_dist.fc_mean.bias"]
    sc = torch.exp(a["act_dist.log_std"])
    lsc = torch.log(sc)
    act = loc + sc * torch.as_tensor(np.asarray(eps)).to(f32) if eps is not None else loc
    d = act - loc
    lp = None
    for o in range(4):
        k = 0 if defect == "log_std_of_component_0" else o
        term = (-(d[..., o] * d[..., o]) / (2.0 * (sc[k] * sc[k])) - lsc[k]) - 0.91893853320467274
        lp = term if lp is None else lp + term
    return loc, lp.unsqueeze(-1)


def emulate_kernel(actor, critic, obs, eps, defect=None):
    """[loc, log_prob, value] as fp32 torch statements of hns_policy_forward_kernel's ALGORITHM (csrc/hns_policy.hip), not of the reference's
    statements: single-query algebra (W_k^T q / sqrt(128) with the key bias dropped, W_v (sum_j a_j t_j) + b_v), the online softmax in token
    order seeded by token 0 with l = 1, two-pass LayerNorm with 1 / sqrt(var + 1e-5), exact-erf GELU, the log-probability summed in component
    order.  (The order of the additions inside a dot product is torch's, not the MFMA's: fp32 noise either way.)  eps None: the mode.
    `defect` seeds one subtle error (DEFECTS) into both networks."""
    assert defect is None or defect in DEFECTS, defect
    a, c = _f32_params(actor), _f32_params(critic)
    obs = {k: torch.as_tensor(np.asarray(v)).to(torch.float32) for k, v in obs.items()}
    with torch.no_grad():
        loc, lp = emulate_head(a, _emulate_encoder(a, "encoder.", obs, defect), eps, defect)
        value = _emulate_encoder(c, "base.", obs, defect) @ c["v_out.weight"].T + c["v_out.bias"]
    return [loc.numpy(), lp.numpy(), value.numpy()]


# the seeded defects of emulate_kernel: each must fail the gate on a committed case (test_policy_net.py names it)
DEFECTS = ("softmax_rescale_omitted", "layernorm_eps_0", "score_scale_bf16", "gelu_tanh", "value_bias_dropped", "last_cylinder_skipped",
           "others_with_cylinder_bias", "log_std_of_component_0")


def philox_normal(seed, counter, rows, dtype=np.float64):
    """[rows, 4] standard normals as include/hns.h and DESIGN 7.3 state them: Philox4x32-10 with key `seed` (low, high word) and counter
    (call counter low, high, row low, high), Box-Muller on both pairs: u1 = ((x >> 8) + 1) 2^-24 in (0, 1], u2 = (y >> 8) 2^-24 in [0, 1),
    components (r cos, r sin) with r = sqrt(-2 log u1) and the angle 2 pi u2.  dtype float32 multiplies and evaluates in fp32 throughout."""
    import hns_oracle as O
    dt = np.dtype(dtype).type
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    w = np.array([O.philox(seed & 0xffffffff, seed >> 32, counter & 0xffffffff, counter >> 32, r & 0xffffffff, r >> 32) for r in range(rows)],
                 dtype=np.uint32).reshape(rows, 2, 2)
    u1 = ((w[..., 0] >> 8) + 1).astype(dtype) * dt(2.0 ** -24)
    u2 = (w[..., 1] >> 8).astype(dtype) * dt(2.0 ** -24)
    rad = np.sqrt(dt(-2.0) * np.log(u1))
    ang = dt(2.0 * math.pi) * u2
    out = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).reshape(rows, 4)
    assert out.dtype == np.dtype(dtype)
    return out
