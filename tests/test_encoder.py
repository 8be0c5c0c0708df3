"""The encoder as a differentiable op (hns_amd.encoder) on the CPU: the C entries exist, the module carries the reference's names, the CPU
path is the restatement the other modules run, and every refusal is raised.  The device kernels: tests/test_hip_encoder.py.

Gradient gate (the project's rule, BAR = 8): for each of the 20 gradient tensors of (encode(...) * dy).sum(), e_cpu <= 8 max(e_32, 2^-24
max|g_64|), errors as max-abs against fp64 autograd of tests/policy_reference.py's encoder, e_32 the error of the same statements in fp32."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import policy_reference as R
from hns_amd import abi
from hns_amd import encoder as EN
from hns_amd import policy as P

BAR = 8.0
HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("hns_encoder_workspace_bytes", "hns_encoder_forward", "hns_encoder_backward")


def _case(A, K, D, S, seed):
    """(encoder parameters by field, reference-named critic dict, obs as tensors) of a random network and batch."""
    _, critic = R.random_net(D, A, seed)
    obs, _ = R.random_obs(S, A, K, D, seed + 1)
    p = {f: torch.as_tensor(critic["base." + k]) for k, f in P._ENCODER.items() if "base." + k in critic}
    o = {k: torch.as_tensor(v) for k, v in obs.items()}
    return p, critic, o


def test_library_exports_and_declares_the_encoder_entries():
    lib = ctypes.CDLL(abi.library_path())
    for sym in NEW:
        getattr(lib, sym)
        assert sym in abi.EXPORTED_SYMBOLS
    lib = abi.load_library()
    assert len(lib.hns_encoder_forward.argtypes) == 9 and len(lib.hns_encoder_backward.argtypes) == 10
    size = lib.hns_encoder_workspace_bytes
    assert size.restype is ctypes.c_size_t
    fwd, bwd = size(96, 35, 3, 5, 0), size(96, 35, 3, 5, 1)
    assert 0 < fwd < bwd <= lib.hns_critic_train_workspace_bytes(96, 35, 3, 5)
    assert fwd % 256 == 0 and bwd % 256 == 0
    assert bwd - fwd >= 12 * 96 * 128 * 4                       # the staged operand pairs are the backward pass' alone
    for rows, D, A, K in ((0, 35, 3, 5), (-1, 35, 3, 5), (96, 0, 3, 5), (96, 97, 3, 5), (96, 35, 0, 5), (96, 35, 8, 5), (96, 35, 3, 0), (96, 35, 3, 17),
                          (2 ** 31, 35, 3, 5)):
        assert size(rows, D, A, K, 0) == 0 and size(rows, D, A, K, 1) == 0, (rows, D, A, K)


@pytest.mark.parametrize("tag", ["a3k5d35", "a1k5d20"])
def test_module_state_dict_has_exactly_the_reference_names(tag):
    z = np.load(os.path.join(HERE, "golden", "g_policy.npz"))
    actor, critic, obs, _, _ = R.golden_case(z, tag)
    strip = lambda k: k[len("module."):] if k.startswith("module.") else k
    want_a = {strip(k)[len("encoder."):] for k in actor if strip(k).startswith("encoder.")}
    want_c = {strip(k)[len("base."):] for k in critic if strip(k).startswith("base.")}
    A, D = obs["state_self"].shape[1], obs["state_self"].shape[-1]
    enc = EN.AttentionEncoder(D, A)
    assert set(enc.state_dict()) == want_a == want_c
    assert len(want_a) == (20 if A > 1 else 18)
    for k, v in enc.state_dict().items():
        assert tuple(v.shape) == tuple(actor[[n for n in actor if strip(n) == "encoder." + k][0]].shape), k
    # initialised as policy.random_parameters initialises an encoder
    ref, _ = P.random_parameters(D, A, 0)
    assert all(torch.equal(v, ref["encoder." + k]) for k, v in enc.state_dict().items())


def test_from_reference_round_trips_bit_for_bit():
    actor, critic = P.random_parameters(24, 3, 5)
    for prefix, src in (("encoder.", actor), ("base.", critic)):
        enc = EN.AttentionEncoder.from_reference({"module." + k: v for k, v in src.items()}, prefix)
        sd = enc.state_dict()
        want = {k[len(prefix):]: v for k, v in src.items() if k.startswith(prefix)}
        assert list(sd) == [k for k in P._ENCODER if k in want] and set(sd) == set(want)      # the reference's registration order as well
        assert all(torch.equal(sd[k], want[k]) for k in want)
        assert all(sd[k].data_ptr() != want[k].data_ptr() for k in want)          # copied
    # a MAPPOPolicy.state_dict() checkpoint, nested as it is saved; and a module
    ckpt = {"actor_params": {"module": {"encoder": {k[len("encoder."):]: v for k, v in actor.items() if k.startswith("encoder.")}}}, "critic": critic}
    a, c = EN.AttentionEncoder.from_reference(ckpt, "encoder."), EN.AttentionEncoder.from_reference(ckpt, "base.")
    assert torch.equal(a.attn.in_proj_weight, actor["encoder.attn.in_proj_weight"]) and torch.equal(c.linear2.bias, critic["base.linear2.bias"])
    again = EN.AttentionEncoder.from_reference(torch.nn.ModuleDict({"base": c}), "base.")
    assert all(torch.equal(v, c.state_dict()[k]) for k, v in again.state_dict().items())
    one = EN.AttentionEncoder.from_reference(P.random_parameters(20, 1, 3)[1], "base.")
    assert not one.has_others and "split_embed.embed.state_others.weight" not in one.state_dict()
    with pytest.raises(P.PolicyConfigError, match="no PartialAttentionEncoder"):
        EN.AttentionEncoder.from_reference(actor, "base.")


@pytest.mark.parametrize("shape", [(3, 5, 35), (1, 5, 20)])
def test_cpu_forward_is_the_policy_restatement_bit_for_bit(shape):
    A, K, D = shape
    p, critic, o = _case(A, K, D, 19, 40 + A)
    cp = P.parse_parameters({k: torch.as_tensor(v) for k, v in critic.items()}, P.CRITIC_NAMES, "critic")
    want = P.torch_forward(None, cp, o["state_self"], o.get("state_others"), o["cylinders"], value_only=True).value
    feats = EN.encode(p, o["state_self"], o.get("state_others"), o["cylinders"])
    assert tuple(feats.shape) == (19, A, 128)
    assert torch.equal(F.linear(feats, cp["head_w"], cp["head_b"]), want)
    # parse_parameters' dict with its head is taken as it is; the rollout layout with an index reads the same rows
    idx = torch.tensor([7, 0, 18, 3])
    lay = lambda t: t.reshape(1, 19, *t.shape[1:]) if t is not None else None
    sub = EN.encode(cp, lay(o["state_self"]), lay(o.get("state_others")), lay(o["cylinders"]), idx)
    gathered = EN.encode(p, o["state_self"][idx], o["state_others"][idx] if A > 1 else None, o["cylinders"][idx])
    assert torch.equal(sub, gathered)                           # (CPU BLAS rounds a 4-row product differently from a 19-row one: no feats[idx])
    assert torch.allclose(sub, feats[idx], atol=1e-5)
    mod = EN.AttentionEncoder.from_reference({k: torch.as_tensor(v) for k, v in critic.items()}, "base.")
    assert torch.equal(mod(o["state_self"], o.get("state_others"), o["cylinders"]), feats)


@pytest.mark.parametrize("shape", [(3, 5, 35), (1, 5, 20), (6, 16, 24)])
def test_cpu_gradients_pass_the_fp64_gate(shape):
    A, K, D = shape
    p, critic, o = _case(A, K, D, 13, 60 + A)
    dy = torch.randn(13, A, 128, generator=torch.Generator().manual_seed(3))

    def ref(dtype):
        q = {k: torch.as_tensor(v).to(dtype).requires_grad_(True) for k, v in critic.items() if k.startswith("base.")}
        (R.encoder(q, "base.", o, dtype) * dy.to(dtype)).sum().backward()
        return {P._ENCODER[k[len("base."):]]: v.grad.double().numpy() for k, v in q.items()}

    r64, r32 = ref(torch.float64), ref(torch.float32)
    leaves = {f: t.clone().requires_grad_(True) for f, t in p.items()}
    (EN.encode(leaves, o["state_self"], o.get("state_others"), o["cylinders"]) * dy).sum().backward()
    assert set(leaves) == set(r64)
    for f, t in leaves.items():
        h, a, b = t.grad.double().numpy(), r64[f], r32[f]
        assert h.shape == a.shape and np.isfinite(h).all(), f
        e, e32 = np.abs(h - a).max(), np.abs(b - a).max()
        bound = max(e32, 2.0 ** -24 * np.abs(a).max())
        print(f"  a{A}k{K}d{D} {f}: e_cpu {e:.3e} e_32 {e32:.3e} ratio {e / bound:.2f}")
        assert e <= BAR * bound, (f, e, bound)
    # the gradients are views of ONE allocation
    got = torch.autograd.grad((EN.encode(leaves, o["state_self"], o.get("state_others"), o["cylinders"]) * dy).sum(), list(leaves.values()))
    assert len({g.untyped_storage().data_ptr() for g in got}) == 1
    assert all(torch.equal(g, t.grad) for g, t in zip(got, leaves.values()))


def test_autograd_semantics_on_the_cpu():
    p, _, o = _case(3, 5, 20, 6, 80)
    args = (o["state_self"], o["state_others"], o["cylinders"])
    with torch.no_grad():
        plain = EN.encode({f: t.clone().requires_grad_(True) for f, t in p.items()}, *args)
    assert plain.grad_fn is None and not plain.requires_grad
    assert EN.encode(p, *args).grad_fn is None                  # no parameter requires grad: nothing to save
    leaves = {f: t.clone().requires_grad_(f != "ln_b") for f, t in p.items()}
    out = EN.encode(leaves, *args)
    assert torch.equal(out, plain)
    out.sum().backward()
    assert leaves["ln_b"].grad is None and all(t.grad is not None for f, t in leaves.items() if f != "ln_b")
    once = {f: t.grad.clone() for f, t in leaves.items() if f != "ln_b"}
    EN.encode(leaves, *args).sum().backward()
    assert all(torch.equal(leaves[f].grad, once[f] + once[f]) for f in once)
    assert leaves["in_proj_b"].grad[128:256].abs().max() < 1e-5   # the key bias: the softmax cancels it (exactly zero on the device)


def test_refusals():
    p, _, o = _case(3, 5, 20, 6, 90)
    xs, xo, xc = o["state_self"], o["state_others"], o["cylinders"]
    leaves = {f: t.clone().requires_grad_(True) for f, t in p.items()}
    with pytest.raises(ValueError, match="observation gradients are not provided"):
        EN.encode(leaves, xs.clone().requires_grad_(True), xo, xc)
    with pytest.raises(ValueError, match="observation gradients are not provided"):
        EN.encode(leaves, xs, xo, xc.clone().requires_grad_(True))
    with pytest.raises(TypeError, match="float32"):
        EN.encode(leaves, xs.double(), xo, xc)
    with pytest.raises(TypeError, match="float32"):
        EN.encode({**p, "norm1_w": p["norm1_w"].double()}, xs, xo, xc)
    with pytest.raises(ValueError, match="share one device"):
        EN.encode(leaves, xs.to("meta"), xo, xc)
    with pytest.raises(ValueError, match="state_self rows have"):
        EN.encode(leaves, xs[..., :19], xo, xc)
    with pytest.raises(ValueError, match="state_others"):
        EN.encode(leaves, xs, None, xc)
    with pytest.raises(ValueError, match="cylinders must be"):
        EN.encode(leaves, xs, xo, xc[..., :4])
    with pytest.raises(ValueError, match="must be"):
        EN.encode({**p, "linear1_w": p["linear1_w"][:64]}, xs, xo, xc)
    with pytest.raises(ValueError, match="missing parameters"):
        EN.encode({f: t for f, t in p.items() if f != "norm2_b"}, xs, xo, xc)
    with pytest.raises(ValueError, match="does not have"):
        EN.encode({**p, "rnn_w": p["ln_w"]}, xs, xo, xc)
    lay = lambda t: t.reshape(2, 3, *t.shape[1:])
    for bad in ([0, 6], [-1, 2]):
        with pytest.raises(IndexError, match="outside the 6 env-steps"):
            EN.encode(leaves, lay(xs), lay(xo), lay(xc), torch.tensor(bad))
    with pytest.raises(TypeError, match="int64"):
        EN.encode(leaves, lay(xs), lay(xo), lay(xc), torch.tensor([0, 1], dtype=torch.int32))
    # torch's own errors: a second backward through the freed node, a parameter stepped in between, double backward
    out = EN.encode(leaves, xs, xo, xc).sum()
    out.backward()
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        out.backward()
    out = EN.encode(leaves, xs, xo, xc).sum()
    with torch.no_grad():
        leaves["ln_w"].mul_(1.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.backward()
    out = EN.encode(leaves, xs, xo, xc).sum()
    (g,) = torch.autograd.grad(out, [leaves["norm2_w"]], create_graph=True)
    with pytest.raises(RuntimeError, match="does not require grad"):           # no graph behind the gradients
        g.sum().backward()
    w = torch.ones(6, 3, 128, requires_grad=True)
    (g,) = torch.autograd.grad((EN.encode(leaves, xs, xo, xc) * w).sum(), [leaves["norm2_w"]], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
