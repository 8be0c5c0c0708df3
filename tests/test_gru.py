"""The GRU as a differentiable op (hns_amd.rnn) on the CPU: the restatement against the reference's recorded run, the C entries, the module's
names, the CPU node's semantics and every Python refusal.  The device kernels: tests/test_hip_gru.py.

Gradient gate (the project's rule, BAR = 8): for each gradient of (out dy).sum() + (h_last dh).sum() — six parameter tensors, dx, dh0 —
e_cpu <= 8 max(e_32, 2^-24 max|g_64|), errors as max-abs against fp64 autograd of tests/gru_reference.py, e_32 the error of the same
statements in fp32; per PARTITION (gru_reference.gate: the r, z, n thirds of the 384-row tensors, out and dx per step), the bound from the
partition's own e_32 and max|g_64|.

Teeth (the last section): gru_reference.emulate_kernel, an fp32 restatement of the KERNELS' algorithm, passes that gate on every case the
device gate runs, and each of nine seeded defects taken from the kernels' own structure fails it on a named case (DEFECT_TABLE)."""
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
    worst, whole, bad = GR.gate(f"S{S}L{L} cpu", [(name, got[name].double().numpy(), r64[name], r32[name]) for name in GR.GRADS])
    print(f"  S{S} L{L}: worst partition ratio {worst:.2f}, worst whole-tensor ratio {whole:.2f}")
    assert not bad, bad
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


# ---------------------------------------------------------------------------------------------------------------------------------------
# Does the fp64 gate have teeth?  emulate_kernel is an fp32 restatement of the kernels' algorithm; the cases are the ones the GPU gate runs
# (test_hip_gru.py: CASES, the five flag patterns, and (4097, 3) — a second trip of the persistent loops, tps = 2, a ragged last split).
BIG = (4097, 3)
GATE_CASES = [f"S{S}L{L}" for S, L in GR.CASES] + ["flags-" + q for q in GR.FLAG_PATTERNS] + ["S%dL%d" % BIG]


def _items(res, r64, r32):
    (o, h, g), (o64, h64, g64), (o32, h32, g32) = res, r64, r32
    return [("out", o, o64, o32), ("h_last", h, h64, h32)] + [(n, g[n], g64[n], g32[n]) for n in GR.GRADS]


@pytest.fixture(scope="module")
def gate_cases():
    """tag -> (case, names that are identically zero, fp64 reference, fp32 reference) of every case of the GPU gate."""
    cases = {f"S{S}L{L}": (GR.shape_case(S, L), ()) for S, L in GR.CASES}
    cases.update({"flags-" + q: (GR.flag_case(q), GR.FLAG_ZERO.get(q, ())) for q in GR.FLAG_PATTERNS})
    cases["S%dL%d" % BIG] = (GR.shape_case(*BIG), ())
    assert list(cases) == GATE_CASES
    return {k: (c, zero, GR.run(*c, torch.float64), GR.run(*c, torch.float32)) for k, (c, zero) in cases.items()}


def test_the_big_case_reaches_the_branches_the_defects_sit_in():
    pl = GR.plan(*BIG)
    assert pl["tiles"] == GR.MAX_GROUPS + 1 and pl["groups"] == GR.MAX_GROUPS           # workgroup 0 takes a second tile
    assert pl["tps"] == 2 and pl["splits"] * pl["tps"] - pl["wg_tiles"] == 1            # a ragged last split: one tile of two
    assert pl["rows"] - (pl["wg_tiles"] - 1) * GR.WG_ROWS == 3                          # ... with three live rows
    assert all(GR.plan(S, L)["tps"] == 1 and GR.plan(S, L)["tiles"] <= GR.MAX_GROUPS for S, L in GR.CASES + [(18, 4)])


def test_the_kernels_algorithm_in_fp32_passes_the_partition_gate_on_every_case(gate_cases):
    """No defect: the emulation stays under the bar in every partition of every tensor, and is exactly zero where the reference is
    identically zero.  Measured worst ratio: 2.75 per partition (S3L64, dx at one step), 2.42 per whole tensor (S1L16)."""
    worst = whole = 0.0
    for tag, (case, zero, r64, r32) in gate_cases.items():
        w, ww, bad = GR.gate(tag, _items(GR.emulate_kernel(*case), r64, r32), zero=zero, verbose=False)
        print(f"  {tag}: worst partition ratio {w:.2f}, worst whole-tensor ratio {ww:.2f}")
        assert not bad, (tag, bad)
        worst, whole = max(worst, w), max(whole, ww)
    print(f"  emulate_kernel, no defect: worst ratio {worst:.2f} per partition, {whole:.2f} per whole tensor, of {GR.BAR}")


# defect -> the case that must fail the gate with it, and the tensor it fails on.  Measured ratios on the named case and tensor (bar 8), whole
# tensor / worst partition, and the cases that still pass:
#   mask_after_cell              flags-mixed out 1.4e6 / 1.5e6; passes flags-none (nothing to mask)
#   dh_unmasked                  flags-first dh0 inf / inf (an exact zero that is not); passes flags-none
#   hn_from_an                   S16L3 weight_hh 5.0e6 / 5.0e6 (the n third); passes none
#   bhn_outside_r                S37L16 out 3.9e5 / 5.2e5; passes none
#   dar_without_bhn              S33L1 weight_ih 1.8e5 / 1.6e6 (the r third: the whole-tensor bound is the n third's); passes none
#   dx_without_ln_term           S15L2 dx 5.0e6 / 5.5e6; passes none
#   stale_state_second_trip      S4097L3 out 1.0e6 / 1.3e6; no other case has a second trip
#   last_split_dropped           S4097L3 weight_ih 8.7e4 / 1.0e5 (the ragged split: 3 live rows); passes the three cases with one split
#   ln_partials_first_trip_only  S4097L3 ln_w 3.9e4 / 3.9e4; no other case has a second trip
# Every defect is three orders of magnitude past the bar on the whole tensor already: what the partitions add is the margin of the small
# thirds (dar_without_bhn: 9 x), not a defect that only they catch.
DEFECT_TABLE = {
    "mask_after_cell": ("flags-mixed", "out"),
    "dh_unmasked": ("flags-first", "dh0"),
    "hn_from_an": ("S16L3", "weight_hh"),
    "bhn_outside_r": ("S37L16", "out"),
    "dar_without_bhn": ("S33L1", "weight_ih"),
    "dx_without_ln_term": ("S15L2", "dx"),
    "stale_state_second_trip": ("S4097L3", "out"),
    "last_split_dropped": ("S4097L3", "weight_ih"),
    "ln_partials_first_trip_only": ("S4097L3", "ln_w"),
}


def test_the_defect_table_names_every_defect():
    assert set(DEFECT_TABLE) == set(GR.DEFECTS) and len(GR.DEFECTS) == 9
    assert all(tag in GATE_CASES and name in ("out", "h_last") + GR.GRADS for tag, name in DEFECT_TABLE.values())


@pytest.mark.parametrize("defect", GR.DEFECTS)
def test_each_seeded_defect_fails_the_gate_on_its_named_case(gate_cases, defect):
    """A subtly wrong kernel does not pass: the same emulation with ONE defect exceeds the bar on the named case and tensor; the number of
    cases it fails on is printed."""
    tag, name = DEFECT_TABLE[defect]
    case, zero, r64, r32 = gate_cases[tag]
    assert not GR.gate(tag, _items(GR.emulate_kernel(*case), r64, r32), zero=zero, verbose=False)[2]
    item = next(it for it in _items(GR.emulate_kernel(*case, defect=defect), r64, r32) if it[0] == name)
    whole, parts = GR.gate_ratios(*item, zero=name in zero)
    assert max(parts.values()) > GR.BAR, (defect, tag, name, parts)
    failing = [t for t, (c, z, a, b) in gate_cases.items() if GR.gate(t, _items(GR.emulate_kernel(*c, defect=defect), a, b), zero=z, verbose=False)[2]]
    print(f"  {defect}: {tag} {name} whole tensor {whole:.3g}, worst partition {max(parts.values()):.3g}; fails on {len(failing)} of {len(gate_cases)} cases")
