"""The GRU as a differentiable op (hns_amd.rnn) on the CPU: the restatement against the reference's recorded run, the C entries, the module's
names, the CPU node's semantics and every Python refusal.  The device kernels: tests/test_hip_gru.py.

Gradient gate (the project's rule, BAR = 8): for each gradient of (out dy).sum() + (h_last dh).sum() — six parameter tensors, dx, dh0 —
e_cpu <= 8 max(e_32, 2^-24 max|g_64|), errors as max-abs against fp64 autograd of tests/gru_reference.py, e_32 the error of the same
statements in fp32."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gru_reference as GR
from hns_amd import abi
from hns_amd import policy as P
from hns_amd import rnn as RN

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("hns_gru_workspace_bytes", "hns_gru_forward", "hns_gru_backward")
GOLDEN_TOL = 1e-5                                               # the project's golden tolerance (README, "parity")


@pytest.fixture(scope="module")
def gru_golden():
    return np.load(os.path.join(HERE, "golden", "g_gru.npz"))


def _golden_params(z, dtype=torch.float32):
    return {f: torch.as_tensor(z["param:" + k]).to(dtype) for k, f in RN.NAMES.items()}


def _leaves(p):
    return {f: t.clone().requires_grad_(True) for f, t in p.items()}


@pytest.mark.parametrize("tag", ["seq", "step"])
def test_restatement_equals_the_reference_run(gru_golden, tag):
    z = gru_golden
    x, h0, flags = (torch.as_tensor(z[f"{tag}:{k}"]) for k in ("x", "h0", "is_init"))
    x3, f2 = (x, flags) if x.dim() == 3 else (x.unsqueeze(1), flags.unsqueeze(1))
    assert f2.any() and not f2.all() and f2[0, 0]
    dy = torch.as_tensor(z[f"{tag}:dy"]).reshape(x3.shape)
    out, h, grads = GR.run(_golden_params(z), x3, h0, f2, dy, torch.as_tensor(z[f"{tag}:dh"]), torch.float32)
    assert np.abs(out.reshape(x.shape) - z[f"{tag}:out"]).max() <= GOLDEN_TOL
    assert np.abs(h - z[f"{tag}:h"]).max() <= GOLDEN_TOL
    for k, f in RN.NAMES.items():
        want = z[f"{tag}:grad:{k}"]
        got = grads[f][::8] if f.startswith("weight") else grads[f]
        assert got.shape == want.shape and np.abs(got - want).max() <= GOLDEN_TOL * max(1.0, np.abs(want).max()), k
    assert np.abs(grads["dx"].reshape(x.shape) - z[f"{tag}:grad:x"]).max() <= GOLDEN_TOL
    assert np.abs(grads["dh0"] - z[f"{tag}:grad:h0"]).max() <= GOLDEN_TOL


def test_library_exports_and_declares_the_gru_entries():
    lib = ctypes.CDLL(abi.library_path())
    for sym in NEW:
        getattr(lib, sym)
        assert sym in abi.EXPORTED_SYMBOLS
    lib = abi.load_library()
    assert len(lib.hns_gru_forward.argtypes) == 8 and len(lib.hns_gru_backward.argtypes) == 11
    size = lib.hns_gru_workspace_bytes
    assert size.restype is ctypes.c_size_t
    assert size(37, 16, 0) == 0                                 # the forward pass needs none
    bwd = size(37, 16, 1)
    assert bwd % 256 == 0 and bwd >= 37 * 16 * 512 * 4          # the gate gradients
    assert size(1536, 16, 1) > bwd
    for seqs, steps in ((0, 16), (-1, 16), (37, 0), (37, 65), (2 ** 40, 1)):
        assert size(seqs, steps, 1) == 0, (seqs, steps)
    assert abi.HNS_GRU_HIDDEN == 128 and abi.HNS_GRU_MAX_STEPS == 64
    assert ctypes.sizeof(abi.HnsGruNet) == 48 and ctypes.sizeof(abi.HnsGruSeq) == 8 + 24 + 16 + 8 + 16


@pytest.mark.parametrize("tag", ["seq", "step"])
def test_cpu_forward_is_the_restatement_bit_for_bit(gru_golden, tag):
    z = gru_golden
    p = _golden_params(z)
    x, h0, flags = (torch.as_tensor(z[f"{tag}:{k}"]) for k in ("x", "h0", "is_init"))
    x3, f2 = (x, flags) if x.dim() == 3 else (x.unsqueeze(1), flags.unsqueeze(1))
    want_out, want_h = GR.forward(p, x3, h0, f2.float())
    out, h = RN.gru(p, x, h0, flags)
    assert out.shape == x.shape and tuple(h.shape) == (x.shape[0], 128)
    assert torch.equal(out, want_out.reshape(x.shape)) and torch.equal(h, want_h)
    # float flags, the reference's trailing 1, no flags / no state as zeros
    assert torch.equal(RN.gru(p, x, h0, flags.float().unsqueeze(-1))[0], out)
    a, b = RN.gru(p, x), RN.gru(p, x, torch.zeros_like(h0), torch.zeros_like(flags))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # [B, A, L, 128] with an env-level flag is the flat call with the flag repeated per agent
    if x.dim() == 3:
        x4 = torch.randn(2, 3, 4, 128, generator=torch.Generator().manual_seed(1))
        h4, f4 = torch.randn(2, 3, 128, generator=torch.Generator().manual_seed(2)), torch.tensor([[[1, 0, 0, 1]], [[0, 0, 1, 0]]], dtype=torch.bool)
        o4, hl4 = RN.gru(p, x4, h4, f4)
        o3, hl3 = RN.gru(p, x4.reshape(6, 4, 128), h4.reshape(6, 128), f4.expand(2, 3, 4).reshape(6, 4))
        assert tuple(o4.shape) == (2, 3, 4, 128) and tuple(hl4.shape) == (2, 3, 128)
        assert torch.equal(o4.reshape(6, 4, 128), o3) and torch.equal(hl4.reshape(6, 128), hl3)


@pytest.mark.parametrize("shape", [(5, 3), (33, 1), (7, 16)])
def test_cpu_gradients_pass_the_fp64_gate(shape):
    S, L = shape
    p, x, h0, flags, dy, dh = GR.random_case(S, L, 100 + S)
    _, _, r64 = GR.run(p, x, h0, flags, dy, dh, torch.float64)
    _, _, r32 = GR.run(p, x, h0, flags, dy, dh, torch.float32)
    leaves, xl, hl = _leaves(p), x.clone().requires_grad_(True), h0.clone().requires_grad_(True)
    out, h = RN.gru(leaves, xl, hl, flags)
    ((out * dy).sum() + (h * dh).sum()).backward()
    got = {**{f: t.grad for f, t in leaves.items()}, "dx": xl.grad, "dh0": hl.grad}
    for name in GR.GRADS:
        assert np.abs(r64[name]).max() > 0, name
        ok, e, bound = GR.gate(name, got[name].double().numpy(), r64[name], r32[name])
        print(f"  S{S} L{L} {name}: e_cpu {e:.3e} bound {bound:.3e} ratio {e / bound:.2f}")
        assert ok, (name, e, bound)
    # the parameter gradients are views of ONE allocation
    g6 = torch.autograd.grad((RN.gru(leaves, x, h0, flags)[0] * dy).sum(), list(leaves.values()))
    assert len({g.untyped_storage().data_ptr() for g in g6}) == 1


def test_module_state_dict_and_from_reference(gru_golden):
    z = gru_golden
    mod = RN.GRU()
    assert list(mod.state_dict()) == list(RN.NAMES) == [k[len("param:"):] for k in z.files if k.startswith("param:")]
    for k, v in mod.state_dict().items():
        assert tuple(v.shape) == z["param:" + k].shape, k
    # the reference's initialisation: orthogonal weights, LayerNorm at (1, 0)
    for w in (mod.cell.weight_ih, mod.cell.weight_hh):
        assert torch.allclose(w.T @ w, torch.eye(128), atol=1e-5)
    assert torch.equal(mod.layer_norm.weight, torch.ones(128)) and torch.equal(mod.layer_norm.bias, torch.zeros(128))
    with pytest.raises(ValueError, match="input size = hidden size = 128"):
        RN.GRU(64, 128)
    ref = {k: torch.as_tensor(z["param:" + k]) for k in RN.NAMES}
    mod.load_state_dict(ref)
    assert all(torch.equal(v, ref[k]) for k, v in mod.state_dict().items())
    assert all(torch.equal(t, ref[k]) for k, f in RN.NAMES.items() for t in [mod.parameters_by_field()[f]])

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.rnn = mod

    nested = {"module": {"rnn": {"cell": {k.split(".")[1]: v for k, v in ref.items() if k.startswith("cell.")},
                                 "layer_norm": {k.split(".")[1]: v for k, v in ref.items() if k.startswith("layer_norm.")}}}}
    sources = {"state_dict": {"module.rnn." + k: v for k, v in ref.items()}, "module": Holder(), "tensordict": nested,
               "checkpoint": {"actor_params": nested, "critic": {}}}
    for kind, src in sources.items():
        got = RN.GRU.from_reference(src)
        assert all(torch.equal(v, ref[k]) for k, v in got.state_dict().items()), kind
        assert all(v.data_ptr() != ref[k].data_ptr() for k, v in got.state_dict().items()), kind      # copied
    assert all(torch.equal(v, ref[k]) for k, v in RN.GRU.from_reference(ref, prefix="").state_dict().items())
    with pytest.raises(P.PolicyConfigError, match="no GRU under"):
        RN.GRU.from_reference({"encoder.ln.weight": torch.ones(128)})
    # the reference's call shape: (output, h) with h padded to the sequence length; a padded h is taken at its first step
    x, h0, flags = (torch.as_tensor(z[f"seq:{k}"]) for k in ("x", "h0", "is_init"))
    out, h = mod(x, h0, flags.unsqueeze(-1))
    assert tuple(h.shape) == (5, 3, 128) and np.abs(out.detach().numpy() - z["seq:out"]).max() <= GOLDEN_TOL
    assert np.abs(h[:, 1].detach().numpy() - z["seq:h"]).max() <= GOLDEN_TOL
    assert torch.equal(mod(x, h0.unsqueeze(1).expand(5, 3, 128), flags)[0], out)
    o1, h1 = mod(torch.as_tensor(z["step:x"]), torch.as_tensor(z["step:h0"]), torch.as_tensor(z["step:is_init"]).unsqueeze(-1))
    assert tuple(h1.shape) == (33, 128) and np.abs(o1.detach().numpy() - z["step:out"]).max() <= GOLDEN_TOL


def test_autograd_semantics_on_the_cpu():
    p, x, h0, flags, dy, dh = GR.random_case(4, 3, 7)
    with torch.no_grad():
        plain = RN.gru(_leaves(p), x, h0, flags)
    assert all(t.grad_fn is None and not t.requires_grad for t in plain)
    assert RN.gru(p, x, h0, flags)[0].grad_fn is None           # nothing requires grad: nothing to save
    leaves = {f: t.clone().requires_grad_(f != "ln_b") for f, t in p.items()}
    xl = x.clone().requires_grad_(True)
    out, h = RN.gru(leaves, xl, h0, flags)
    assert torch.equal(out, plain[0]) and torch.equal(h, plain[1])
    ((out * dy).sum() + (h * dh).sum()).backward()
    assert leaves["ln_b"].grad is None and all(t.grad is not None for f, t in leaves.items() if f != "ln_b")
    assert xl.grad is not None and xl.grad.shape == x.shape
    once = {f: t.grad.clone() for f, t in leaves.items() if f != "ln_b"}
    out, h = RN.gru(leaves, xl, h0, flags)
    ((out * dy).sum() + (h * dh).sum()).backward()
    assert all(torch.equal(leaves[f].grad, once[f] + once[f]) for f in once)
    # only x requires grad (a frozen GRU behind a training encoder); only h_last is used
    xo = x.clone().requires_grad_(True)
    RN.gru(p, xo, h0, flags)[1].sum().backward()
    assert xo.grad is not None and xo.grad.abs().max() > 0
    # dh0 of a sequence that starts an episode is zero
    hl = h0.clone().requires_grad_(True)
    f0 = flags.clone()
    f0[:, 0] = torch.tensor([True, False, True, False])
    RN.gru(p, x, hl, f0)[0].sum().backward()
    assert (hl.grad[0] == 0).all() and (hl.grad[2] == 0).all() and hl.grad[1].abs().max() > 0
    # torch's own errors: a second backward through the freed node, a parameter stepped in between, double backward
    loss = RN.gru(leaves, x, h0, flags)[0].sum()
    loss.backward()
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        loss.backward()
    loss = RN.gru(leaves, x, h0, flags)[0].sum()
    with torch.no_grad():
        leaves["ln_w"].mul_(1.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    w = torch.ones(4, 3, 128, requires_grad=True)
    (g,) = torch.autograd.grad((RN.gru(leaves, x, h0, flags)[0] * w).sum(), [leaves["weight_hh"]], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_refusals():
    p, x, h0, flags, _, _ = GR.random_case(4, 3, 9)
    with pytest.raises(TypeError, match="float32"):
        RN.gru(p, x.double(), h0, flags)
    with pytest.raises(TypeError, match="float32"):
        RN.gru({**p, "ln_w": p["ln_w"].double()}, x, h0, flags)
    with pytest.raises(TypeError, match="float32"):
        RN.gru(p, x, h0.double(), flags)
    with pytest.raises(TypeError, match="must be a tensor"):
        RN.gru(p, x.numpy(), h0, flags)
    with pytest.raises(ValueError, match="must be"):
        RN.gru(p, x[..., :127], h0, flags)                      # last dimension != 128
    with pytest.raises(ValueError, match="must be"):
        RN.gru(p, x.reshape(1, 1, 4, 3, 128), None, None)
    with pytest.raises(ValueError, match="must be"):
        RN.gru(p, x[0, 0], None, None)
    with pytest.raises(ValueError, match=r"sequence length must be in \[1, 64\]"):
        RN.gru(p, torch.zeros(2, 65, 128))
    with pytest.raises(ValueError, match="no sequences"):
        RN.gru(p, torch.zeros(0, 3, 128))
    with pytest.raises(ValueError, match="share one device"):
        RN.gru(p, x.to("meta"), None, None)
    with pytest.raises(ValueError, match="share one device"):
        RN.gru(p, x, h0.to("meta"), None)
    with pytest.raises(ValueError, match="h0 must be"):
        RN.gru(p, x, h0[:3], flags)
    with pytest.raises(ValueError, match="is_init must have"):
        RN.gru(p, x, h0, flags[:, :2])
    with pytest.raises(ValueError, match="weight_hh must be"):
        RN.gru({**p, "weight_hh": p["weight_hh"][:256]}, x, h0, flags)
    with pytest.raises(ValueError, match="contiguous"):
        RN.gru({**p, "weight_ih": p["weight_ih"].T.contiguous().T.reshape(128, 384).T}, x, h0, flags)
    with pytest.raises(ValueError, match="missing parameters"):
        RN.gru({f: t for f, t in p.items() if f != "ln_b"}, x, h0, flags)
    with pytest.raises(ValueError, match="does not have"):
        RN.gru({**p, "weight_ho": p["ln_w"]}, x, h0, flags)
    with pytest.raises(TypeError, match="must map"):
        RN.gru(list(p.values()), x, h0, flags)
