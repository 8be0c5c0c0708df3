"""The GRU block (include/hns.h: hns_gru_*; modules/rnn.py:44-89 with nn.GRUCell's statements) restated in torch at a given dtype, with autograd:
the reference of tests/test_gru.py (fp32: the golden fixture, the CPU node's bits) and tests/test_hip_gru.py (fp64: the accuracy gate).

    for t = 0 .. L - 1:  h <- h (1 - is_init[:, t]);  r, z = sigmoid(W_i{r,z} x_t + b_i{r,z} + W_h{r,z} h + b_h{r,z});
                         n = tanh(W_in x_t + b_in + r (W_hn h + b_hn));  h <- (1 - z) n + z h
    out = LayerNorm(stack(h) + x);  h_last = h

This is the project's own restatement; tests/golden/make_golden_gru.py executes the reference's class for the fixture."""
import numpy as np
import torch
import torch.nn.functional as F

H = 128
FIELDS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh", "ln_w", "ln_b")
GRADS = FIELDS + ("dx", "dh0")


def forward(p, x, h0, is_init):
    """p: {field: tensor}; x [S, L, 128]; h0 [S, 128]; is_init [S, L] of 0 / 1 in x's dtype -> (out [S, L, 128], h_last [S, 128])."""
    h, outs = h0, []
    for t in range(x.shape[1]):
        h = h * (1 - is_init[:, t:t + 1])
        gi, gh = F.linear(x[:, t], p["weight_ih"], p["bias_ih"]), F.linear(h, p["weight_hh"], p["bias_hh"])
        i_r, i_z, i_n = gi.chunk(3, 1)
        h_r, h_z, h_n = gh.chunk(3, 1)
        r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
        n = torch.tanh(i_n + r * h_n)
        h = (1 - z) * n + z * h
        outs.append(h)
    return F.layer_norm(torch.stack(outs, 1) + x, (H,), p["ln_w"], p["ln_b"], 1e-5), h


def random_case(S, L, seed, flag_p=0.15, first_flag=None):
    """The accuracy gate's inputs (fp32 CPU tensors): orthogonal weights, biases 0.1 N(0, 1), LN weight 1 + 0.1 N, x ~ N(0, 1), h0 ~ 0.5 N, flags
    Bernoulli(flag_p), seeded dy and dh.  first_flag: is_init[0, 0] forced to it."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    p = {}
    for f in ("weight_ih", "weight_hh"):
        q, _ = torch.linalg.qr(rn(3 * H, H))                    # [384, 128] with orthonormal columns: what nn.init.orthogonal_ makes
        p[f] = q.contiguous()
    p["bias_ih"], p["bias_hh"] = 0.1 * rn(3 * H), 0.1 * rn(3 * H)
    p["ln_w"], p["ln_b"] = 1.0 + 0.1 * rn(H), 0.1 * rn(H)
    x, h0 = rn(S, L, H), 0.5 * rn(S, H)
    flags = (torch.rand(S, L, generator=g) < flag_p)
    if first_flag is not None:
        flags[0, 0] = bool(first_flag)
    return p, x, h0, flags, rn(S, L, H), rn(S, H)


def run(p, x, h0, flags, dy, dh, dtype):
    """(out, h_last, {gradient name: array}) of sum(out dy) + sum(h_last dh) at `dtype`, as fp64 numpy."""
    q = {f: t.detach().to(dtype).requires_grad_(True) for f, t in p.items()}
    xl, hl = x.detach().to(dtype).requires_grad_(True), h0.detach().to(dtype).requires_grad_(True)
    out, h = forward(q, xl, hl, flags.to(dtype))
    ((out * dy.to(dtype)).sum() + (h * dh.to(dtype)).sum()).backward()
    grads = {f: q[f].grad.double().numpy() for f in FIELDS}
    grads["dx"], grads["dh0"] = xl.grad.double().numpy(), hl.grad.double().numpy()
    return out.detach().double().numpy(), h.detach().double().numpy(), grads


def gate(name, got, r64, r32, bar=8.0):
    """The project's rule: e <= bar max(e_32, 2^-24 max|ref_64|), max-abs errors against fp64.  -> (passes, e, bound)."""
    got = np.asarray(got, np.float64)
    assert got.shape == r64.shape and np.isfinite(got).all(), name
    e, e32 = np.abs(got - r64).max(), np.abs(r32 - r64).max()
    bound = max(e32, 2.0 ** -24 * np.abs(r64).max())
    return e <= bar * bound, e, bound
