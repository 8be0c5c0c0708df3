"""The GRU as a differentiable op on the device (hns_gru_forward / hns_gru_backward through hns_amd.rnn) on an MI355X.

Accuracy gate (the rule of test_hip_encoder.py, test_hip_critic_train.py and test_tp_train.py, BAR = 8): for out, h_last, dx, dh0 and EACH of
the six parameter gradients of sum(out dy) + sum(h_last dh), e_hip <= 8 max(e_32, 2^-24 max|ref_64|), errors as max-abs against
tests/gru_reference.py in fp64, e_32 the error of the same statements in CPU fp32.  Inputs: gru_reference.random_case (orthogonal weights,
biases 0.1 N, LN weight 1 + 0.1 N, x ~ N, h0 ~ 0.5 N, flags Bernoulli(0.15), seeded dy and dh; S = 1 runs with is_init[0, 0] = 0, or its dh0
is identically zero).  Every case asserts first, on the CPU, that no fp64 reference tensor is identically zero.  The kernels' sequence tile
is 16: S = 17 and S = 33 are one more than one and two tiles.  Worst measured ratio per case: printed by test_report_ratios (RATIOS).

Measured on an MI355X (worst e_hip / max(e_32, 2^-24 max|ref_64|) over a case's ten tensors: out, h_last, dx, dh0, six parameter gradients):
  (S, L): (37, 16) 1.50, (1, 16) 1.83, (15, 2) 1.36, (16, 3) 1.56, (17, 1) 1.53, (33, 1) 1.43, (5, 17) 1.50, (3, 64) 1.60;
  flag patterns at (18, 4): first step 1.55, last step 1.59, all 1.59, none 1.65, mixed 1.92;
  encode -> gru -> nn.Linear(128, 1) (values, the head's 2, the GRU's 6 and the encoder's 20 gradient tensors): 1.60."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import gru_reference as GR
import policy_reference as R
from hns_amd import abi
from hns_amd import encoder as EN
from hns_amd import policy as P
from hns_amd import rnn as RN

pytestmark = pytest.mark.gpu

BAR = 8.0
RATIOS = {}
CASES = [(37, 16), (1, 16), (15, 2), (16, 3), (17, 1), (33, 1), (5, 17), (3, 64)]
CANARY = 1234.5
H = 128


@functools.lru_cache(maxsize=None)
def _reference(S, L):
    """One case per shape with its fp64 and fp32 references, computed once: (inputs, {dtype: (out, h_last, gradients)})."""
    case = GR.random_case(S, L, 2000 + 100 * S + L, first_flag=0 if S == 1 else None)
    return case, {dt: GR.run(*case, dt) for dt in (torch.float64, torch.float32)}


def _gate(tag, items):
    """items: (name, device value, fp64 reference, fp32 reference); records the worst ratio under `tag` and asserts the bar."""
    worst, bad = 0.0, []
    for name, h, a, b in items:
        h, a, b = np.asarray(h, np.float64), np.asarray(a, np.float64), np.asarray(b, np.float64)
        assert h.shape == a.shape == b.shape, (name, h.shape, a.shape)
        assert np.isfinite(h).all(), f"{tag} {name}: not finite"
        e_hip, e_32 = float(np.abs(h - a).max()), float(np.abs(b - a).max())
        bound = max(e_32, 2.0 ** -24 * float(np.abs(a).max()))
        ratio = e_hip / bound if bound > 0 else (0.0 if e_hip == 0 else math.inf)
        print(f"  {tag} {name}: e_hip {e_hip:.3e} e_32 {e_32:.3e} max|ref| {np.abs(a).max():.3e} ratio {ratio:.2f}")
        worst = max(worst, ratio)
        if not ratio <= BAR:
            bad.append(f"{name}: e_hip {e_hip:.3e} > {BAR} x {bound:.3e} (ratio {ratio:.2f})")
    RATIOS[tag] = max(worst, RATIOS.get(tag, 0.0))
    assert not bad, f"{tag}: " + "; ".join(bad)


def _run(p, x, h0, flags, dy, dh, grad=True):
    """The op on the device from CPU inputs: (out, h_last, {name: gradient}) as device tensors."""
    q = {f: t.cuda().requires_grad_(grad) for f, t in p.items()}
    xl = x.cuda().requires_grad_(grad)
    hl = h0.cuda().requires_grad_(grad) if h0 is not None else None
    out, h = RN.gru(q, xl, hl, flags.cuda() if flags is not None else None)
    if not grad:
        return out, h, {}
    ((out * dy.cuda()).sum() + (h * dh.cuda()).sum()).backward()
    g = {f: t.grad for f, t in q.items()}
    g["dx"], g["dh0"] = xl.grad, (hl.grad if hl is not None else None)
    return out.detach(), h.detach(), g


@pytest.mark.parametrize("S,L", CASES)
def test_outputs_and_gradients_pass_the_fp64_gate(S, L):
    case, refs = _reference(S, L)
    (o64, h64, g64), (o32, h32, g32) = refs[torch.float64], refs[torch.float32]
    for name, a in [("out", o64), ("h_last", h64), *g64.items()]:
        assert a.any(), f"{name}: the fp64 reference is identically zero, the case gates nothing"
    out, h, g = _run(*case)
    assert tuple(out.shape) == (S, L, H) and tuple(h.shape) == (S, H)
    _gate(f"S{S}L{L}", [("out", out.cpu().numpy(), o64, o32), ("h_last", h.cpu().numpy(), h64, h32)] +
          [(n, g[n].cpu().numpy(), g64[n], g32[n]) for n in GR.GRADS])


def test_strided_view_of_encoder_features_is_the_contiguous_call_bit_for_bit():
    """[B L A, 128] features read in place as [B, A, L, 128]: out, dx and every gradient against the contiguous call."""
    B, A, L = 5, 3, 3
    p, _, _, _, _, _ = GR.random_case(1, 1, 31)
    g = torch.Generator().manual_seed(32)
    buf = torch.randn(B * L * A, H, generator=g)
    h0, flags = 0.5 * torch.randn(B, A, H, generator=g), torch.rand(B, 1, L, generator=g) < 0.3
    dy, dh = torch.randn(B * L * A, H, generator=g), torch.randn(B, A, H, generator=g)
    view = lambda t: t.view(B, L, A, H).transpose(1, 2)
    res = []
    for contiguous in (False, True):
        q = {f: t.cuda().requires_grad_(True) for f, t in p.items()}
        leaf = buf.cuda().requires_grad_(True)
        hl = h0.cuda().requires_grad_(True)
        x4 = view(leaf).contiguous() if contiguous else view(leaf)
        assert x4.is_contiguous() == contiguous
        out, h = RN.gru(q, x4, hl, flags.cuda())
        assert out.stride() == x4.stride() and tuple(h.shape) == (B, A, H)
        ((out * view(dy.cuda())).sum() + (h * dh.cuda()).sum()).backward()
        res.append((out.detach().contiguous(), h.detach(), leaf.grad, hl.grad, {f: t.grad for f, t in q.items()}))
    (o0, h0_, dx0, dh0, g0), (o1, h1, dx1, dh1, g1) = res
    assert torch.equal(o0, o1) and torch.equal(h0_, h1) and torch.equal(dx0, dx1) and torch.equal(dh0, dh1)
    assert all(torch.equal(g0[f], g1[f]) for f in g0)
    # and the [B, A] index is the flat one: sequence s = b A + a, the env-level flag repeated per agent
    x3 = view(buf).reshape(B * A, L, H)
    o3, h3, g3 = _run(p, x3, h0.reshape(B * A, H), flags.expand(B, A, L).reshape(B * A, L), view(dy).reshape(B * A, L, H), dh.reshape(B * A, H))
    assert torch.equal(o3.view(B, A, L, H), o1) and torch.equal(h3.view(B, A, H), h1) and all(torch.equal(g3[f], g1[f]) for f in g1)
    assert torch.equal(g3["dx"].view(B, A, L, H).transpose(1, 2).reshape(B * L * A, H), dx1)


def test_no_state_and_no_flags_are_zeros_bit_for_bit():
    p, x, h0, flags, dy, dh = GR.random_case(19, 4, 41)
    a = _run(p, x, None, None, dy, dh)
    b = _run(p, x, torch.zeros_like(h0), torch.zeros_like(flags), dy, dh)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][n], b[2][n]) for n in GR.GRADS if n != "dh0") and a[2]["dh0"] is None
    c, d = _run(p, x, h0, None, dy, dh), _run(p, x, h0, torch.zeros_like(flags), dy, dh)
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1]) and all(torch.equal(c[2][n], d[2][n]) for n in GR.GRADS)
    assert not torch.equal(a[0], c[0])


@pytest.mark.parametrize("pattern", ["first", "last", "all", "none", "mixed"])
def test_flags(pattern):
    S, L = 18, 4
    p, x, h0, _, dy, dh = GR.random_case(S, L, 51)
    flags = torch.zeros(S, L, dtype=torch.bool)
    if pattern == "first":
        flags[:, 0] = True
    elif pattern == "last":
        flags[:, L - 1] = True
    elif pattern == "all":
        flags[:] = True
    elif pattern == "mixed":
        flags[::3, 0] = True
        flags[1::4, 2] = True
    out, h, g = _run(p, x, h0, flags, dy, dh)
    o64, h64, g64 = GR.run(p, x, h0, flags, dy, dh, torch.float64)
    o32, h32, g32 = GR.run(p, x, h0, flags, dy, dh, torch.float32)
    names = [n for n in GR.GRADS if g64[n].any()]               # (all sequences start an episode: dh0 is identically zero and checked below)
    _gate("flags-" + pattern, [("out", out.cpu().numpy(), o64, o32), ("h_last", h.cpu().numpy(), h64, h32)] +
          [(n, g[n].cpu().numpy(), g64[n], g32[n]) for n in names])
    first = flags[:, 0]
    if first.any():
        assert bool((g["dh0"][first.cuda()] == 0).all()), "dh0 of a sequence that starts an episode must be exactly zero"
        zero = h0.clone()
        zero[first] = 0
        oz, hz, _ = _run(p, x, zero, flags, dy, dh, grad=False)
        assert torch.equal(oz, out) and torch.equal(hz, h)
    if (~first).any():
        assert bool((g["dh0"][(~first).cuda()] != 0).any())


def test_chaining_and_row_independence_bit_for_bit():
    S, L = 17, 5
    p, x, h0, flags, dy, dh = GR.random_case(S, L, 61)
    out, h, g = _run(p, x, h0, flags, dy, dh)
    q = {f: t.cuda() for f, t in p.items()}
    xd, fd, hc = x.cuda(), flags.cuda(), h0.cuda()
    for t in range(L):                                          # collection: one step per call, the state handed on
        o1, hc = RN.gru(q, xd[:, t], hc, fd[:, t])
        assert tuple(o1.shape) == (S, H) and torch.equal(o1, out[:, t]), f"step {t}"
    assert torch.equal(hc, h)
    # the [S, 1, 128] form of the one-step call, and chained three- and two-step calls
    o3, h3 = RN.gru(q, xd[:, :3], h0.cuda(), fd[:, :3])
    o2, h2 = RN.gru(q, xd[:, 3:], h3, fd[:, 3:])
    assert torch.equal(torch.cat([o3, o2], 1), out) and torch.equal(h2, h)
    # a sequence's results do not depend on the other sequences of the call: 3 .. 9 alone (another tile position, another tile count)
    sl = slice(3, 10)
    os_, hs_, gs = _run(p, x[sl], h0[sl], flags[sl], dy[sl], dh[sl])
    assert torch.equal(os_, out[sl]) and torch.equal(hs_, h[sl]) and torch.equal(gs["dx"], g["dx"][sl]) and torch.equal(gs["dh0"], g["dh0"][sl])


def _raw(p, x, h0, flags, dy, dh, fill):
    """hns_gru_forward and hns_gru_backward called directly with canaries around out, h_last, h_hist, dx and dh0 and a workspace filled with
    `fill`: every output as a clone."""
    lib = abi.load_library()
    S, L, _ = x.shape
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x4 = x.cuda().unsqueeze(1)
    init = flags.to(torch.uint8).cuda()
    h0d = h0.cuda()

    def guarded(n):
        t = torch.full((n + 2 * H,), CANARY, device="cuda")
        return t, t[H:H + n]

    (bo, out), (bh, hl), (bhist, hist), (bdx, dx), (bd0, dh0) = guarded(S * L * H), guarded(S * H), guarded(S * L * H), guarded(S * L * H), guarded(S * H)
    dev = {f: t.cuda() for f, t in p.items()}                   # (kept alive: the structs hold bare pointers)
    net, seq = RN._net(dev), RN._seq(x4, h0d, init)
    assert lib.hns_gru_forward(C.byref(net), C.byref(seq), out.data_ptr(), hl.data_ptr(), hist.data_ptr(), None, 0, st) == abi.HNS_OK
    nb = lib.hns_gru_workspace_bytes(S, L, 1)
    ws = torch.empty(nb // 4, dtype=torch.float32, device="cuda").fill_(fill).view(torch.uint8)
    flat = torch.full((RN.grad_layout()[1] + 64,), CANARY, device="cuda")
    grads = RN._views(flat)
    grd = RN._net(grads)
    dyd, dhd = dy.cuda().contiguous(), dh.cuda().contiguous()
    assert lib.hns_gru_backward(C.byref(net), C.byref(seq), hist.data_ptr(), dyd.data_ptr(), dhd.data_ptr(), C.byref(grd), dx.data_ptr(),
                                dh0.data_ptr(), ws.data_ptr(), nb, st) == abi.HNS_OK
    torch.cuda.synchronize()
    del dev
    for name, (buf, n) in {"out": (bo, S * L * H), "h_last": (bh, S * H), "h_hist": (bhist, S * L * H), "dx": (bdx, S * L * H), "dh0": (bd0, S * H)}.items():
        assert bool((buf[:H] == CANARY).all()) and bool((buf[H + n:] == CANARY).all()), f"floats around {name} were written"
        assert bool(torch.isfinite(buf[H:H + n]).all()) and bool((buf[H:H + n] != CANARY).all()), name
    assert bool((flat[-64:] == CANARY).all()) and bool(torch.isfinite(flat[:-64]).all()) and bool((flat[:-64] != CANARY).all())
    return [t.clone() for t in (out, hl, hist, dx, dh0, flat)]


def test_determinism_workspace_from_scratch_and_canaries():
    S, L = 21, 6                                                # two tiles, the second with five live sequences
    case = GR.random_case(S, L, 71)
    runs = [_raw(*case, fill) for fill in (0.0, float("nan"), 0.0)]
    names = ("out", "h_last", "h_hist", "dx", "dh0", "gradients")
    for k, r in enumerate(runs[1:]):
        differ = [(n, float((a - b).abs().max()), int((a != b).sum())) for n, a, b in zip(names, r, runs[0]) if not torch.equal(a, b)]
        assert not differ, f"run {k + 1} against run 0 (name, max difference, values): {differ}"
    # the hidden states the forward pass leaves: h_hist[:, L - 1] is h_last; and the direct calls are the module's
    out, h, g = _run(*case)
    o, hl, hist, dx, dh0, flat = runs[0]
    assert torch.equal(hist.view(S, L, H)[:, L - 1], hl.view(S, H))
    assert torch.equal(o.view(S, L, H), out) and torch.equal(hl.view(S, H), h) and torch.equal(dx.view(S, L, H), g["dx"]) and torch.equal(dh0.view(S, H), g["dh0"])
    views = RN._views(flat)
    assert all(torch.equal(views[f], g[f]) for f in RN.FIELDS)


def test_autograd_semantics():
    p, x, h0, flags, dy, dh = GR.random_case(9, 3, 81)
    out, h, g1 = _run(p, x, h0, flags, dy, dh)
    dev = {f: t.cuda() for f, t in p.items()}
    xd, hd, fd, dyd, dhd = x.cuda(), h0.cuda(), flags.cuda(), dy.cuda(), dh.cuda()
    # a tensor that does not require grad gets none; the others keep their bits
    leaves = {f: t.clone().requires_grad_(f not in ("ln_w", "weight_hh")) for f, t in dev.items()}
    o, hh = RN.gru(leaves, xd, hd, fd)
    ((o * dyd).sum() + (hh * dhd).sum()).backward()
    assert leaves["ln_w"].grad is None and leaves["weight_hh"].grad is None
    assert all(torch.equal(t.grad, g1[f]) for f, t in leaves.items() if t.requires_grad)
    # two passes accumulate to exactly twice one pass; a non-contiguous incoming gradient is laid out as x
    leaves = {f: t.clone().requires_grad_(True) for f, t in dev.items()}
    wide = torch.zeros(9, 3, 256, device="cuda")
    wide[..., ::2] = dyd
    for _ in range(2):
        o, hh = RN.gru(leaves, xd, hd, fd)
        torch.autograd.backward([o, hh], [wide[..., ::2], dhd])
    assert all(torch.equal(t.grad, g1[f] + g1[f]) for f, t in leaves.items())
    # only out used: dh_last arrives as zeros
    xl = xd.clone().requires_grad_(True)
    (RN.gru(dev, xl, hd, fd)[0] * dyd).sum().backward()
    assert bool(torch.isfinite(xl.grad).all()) and not torch.equal(xl.grad, g1["dx"])
    # no_grad, and nothing requiring grad: no node, the same bits
    with torch.no_grad():
        plain = RN.gru(leaves, xd, hd, fd)
    frozen = RN.gru(dev, xd, hd, fd)
    assert plain[0].grad_fn is None and frozen[0].grad_fn is None and torch.equal(plain[0], out) and torch.equal(frozen[1], h)
    # a parameter changed in place between forward and backward: autograd's version check
    loss = (RN.gru(leaves, xd, hd, fd)[0] * dyd).sum()
    with torch.no_grad():
        leaves["bias_hh"].add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    # the module form with the reference's call shape, an optimiser of torch's own on top
    mod = RN.GRU().cuda()
    mod.load_state_dict({k: dev[f] for k, f in RN.NAMES.items()})
    o, hp = mod(xd, hd, fd.unsqueeze(-1))
    assert torch.equal(o, out) and tuple(hp.shape) == (9, 3, H) and torch.equal(hp[:, 0], h)
    opt = torch.optim.AdamW(mod.parameters(), lr=1e-3, weight_decay=0.01)
    ((o * dyd).sum() + (hp[:, 0] * dhd).sum()).backward()
    assert torch.equal(mod.cell.weight_ih.grad, g1["weight_ih"]) and torch.equal(mod.layer_norm.bias.grad, g1["ln_b"])
    opt.step()
    assert not torch.equal(mod(xd, hd, fd)[0], out)
    with pytest.raises(ValueError, match="share one device"):
        RN.gru(dev, x, hd, fd)


def test_composition_encode_gru_linear_passes_the_fp64_gate():
    """encode -> gru -> nn.Linear(128, 1) on five 3-step segments (A 3, K 5, D 35): the head's, the GRU's and the encoder's gradients against
    policy_reference.encoder + gru_reference in fp64.  The features [B L A, 128] are read in place as [B, A, L, 128] and dx is the encoder's
    d features."""
    A, K, D, B, L = 3, 5, 35, 5, 3
    _, critic = R.random_net(D, A, 91)
    obs, _ = R.random_obs(B * L, A, K, D, 92)
    o = {k: torch.as_tensor(v) for k, v in obs.items()}
    p, _, _, _, _, _ = GR.random_case(1, 1, 93)
    g = torch.Generator().manual_seed(94)
    h0, flags = 0.5 * torch.randn(B * A, H, generator=g), torch.rand(B, 1, L, generator=g) < 0.3
    hw, hb, dv = 0.1 * torch.randn(1, H, generator=g), torch.randn(1, generator=g), torch.randn(B, A, L, 1, generator=g)
    fl = flags.expand(B, A, L).reshape(B * A, L)

    def ref(dtype):
        q = {k: torch.as_tensor(v).to(dtype).requires_grad_(True) for k, v in critic.items() if k.startswith("base.")}
        r = {f: t.clone().to(dtype).requires_grad_(True) for f, t in p.items()}
        w, b = hw.clone().to(dtype).requires_grad_(True), hb.clone().to(dtype).requires_grad_(True)
        feats = R.encoder(q, "base.", o, dtype)                 # [B L, A, 128]
        x = feats.reshape(B, L, A, H).transpose(1, 2).reshape(B * A, L, H)
        out, _ = GR.forward(r, x, h0.to(dtype), fl.to(dtype))
        v = torch.nn.functional.linear(out, w, b)
        (v * dv.reshape(B * A, L, 1).to(dtype)).sum().backward()
        res = {"values": v.detach().double().numpy(), "head_w": w.grad.double().numpy(), "head_b": b.grad.double().numpy()}
        res.update({"gru." + f: t.grad.double().numpy() for f, t in r.items()})
        res.update({"enc." + P._ENCODER[k[len("base."):]]: t.grad.double().numpy() for k, t in q.items()})
        return res

    r64, r32 = ref(torch.float64), ref(torch.float32)
    for n, a in r64.items():
        assert a.any() or n == "enc.in_proj_b", n
    ep = {f: torch.as_tensor(critic["base." + k]).cuda().requires_grad_(True) for k, f in P._ENCODER.items() if "base." + k in critic}
    gp = {f: t.cuda().requires_grad_(True) for f, t in p.items()}
    head = nn.Linear(H, 1).cuda()
    with torch.no_grad():
        head.weight.copy_(hw)
        head.bias.copy_(hb)
    feats = EN.encode(ep, o["state_self"].cuda(), o["state_others"].cuda(), o["cylinders"].cuda())
    x4 = feats.view(B, L, A, H).transpose(1, 2)
    out, _ = RN.gru(gp, x4, h0.cuda(), flags.cuda())
    assert out.stride() == x4.stride()
    v = head(out)
    (v * dv.cuda()).sum().backward()
    got = {"values": v.detach().reshape(B * A, L, 1), "head_w": head.weight.grad, "head_b": head.bias.grad}
    got.update({"gru." + f: t.grad for f, t in gp.items()})
    got.update({"enc." + f: t.grad for f, t in ep.items()})
    assert set(got) == set(r64)
    _gate("composition", [(n, got[n].cpu().numpy(), r64[n], r32[n]) for n in r64])


def test_c_level_refusals_launch_nothing():
    S, L = 5, 3
    p, x, h0, flags, dy, dh = GR.random_case(S, L, 95)
    lib = abi.load_library()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dev = {f: t.cuda() for f, t in p.items()}
    x4, h0d, init = x.cuda().unsqueeze(1), h0.cuda(), flags.to(torch.uint8).cuda()
    out, hl, hist = (torch.full((n + 4,), CANARY, device="cuda") for n in (S * L * H, S * H, S * L * H))
    dx, dh0 = torch.full((S * L * H + 4,), CANARY, device="cuda"), torch.full((S * H + 4,), CANARY, device="cuda")
    flat = torch.full((RN.grad_layout()[1],), CANARY, device="cuda")
    dyd, dhd = dy.cuda(), dh.cuda()
    nb = lib.hns_gru_workspace_bytes(S, L, 1)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
    net, grd = RN._net(dev), RN._net(RN._views(flat))

    def seq(**kw):
        s = RN._seq(x4, h0d, init)
        for k, v in kw.items():
            if k.startswith("stride"):
                s.x_stride[int(k[-1])] = v
            else:
                setattr(s, k, v)
        return s

    def fwd(s=None, n=None, o=out.data_ptr(), h=hl.data_ptr(), hh=hist.data_ptr(), w=None):
        return lib.hns_gru_forward(C.byref(n if n is not None else net), C.byref(s if s is not None else seq()), o, h, hh, w, 0, st)

    def bwd(s=None, n=None, gr=None, hh=hist.data_ptr(), d=dyd.data_ptr(), dl=dhd.data_ptr(), x_=dx.data_ptr(), d0=dh0.data_ptr(), w=ws.data_ptr(), wb=nb):
        return lib.hns_gru_backward(C.byref(n if n is not None else net), C.byref(s if s is not None else seq()), hh, d, dl,
                                    C.byref(gr if gr is not None else grd), x_, d0, w, wb, st)

    def net_with(field, value, base=net):
        n = abi.HnsGruNet()
        C.memmove(C.byref(n), C.byref(base), C.sizeof(n))
        setattr(n, field, value)
        return n

    cases = [(lambda: lib.hns_gru_forward(None, C.byref(seq()), out.data_ptr(), hl.data_ptr(), None, None, 0, st), "null pointer"),
             (lambda: lib.hns_gru_backward(C.byref(net), None, hist.data_ptr(), dyd.data_ptr(), None, C.byref(grd), dx.data_ptr(), None, ws.data_ptr(), nb, st),
              "null pointer"),
             (lambda: fwd(n=net_with("weight_hh", None)), "parameter pointers"), (lambda: bwd(n=net_with("ln_b", dev["ln_b"].data_ptr() + 4)), "parameter pointers"),
             (lambda: bwd(gr=net_with("bias_ih", None, grd)), "gradient pointers"), (lambda: bwd(gr=net_with("weight_ih", flat.data_ptr() + 8, grd)), "gradient pointers"),
             (lambda: fwd(seq(x=None)), "x must be"), (lambda: bwd(seq(x=x4.data_ptr() + 4)), "x must be"),
             (lambda: fwd(seq(steps=0)), "steps must be in [1, 64]"), (lambda: fwd(seq(steps=65)), "steps must be in [1, 64]"),
             (lambda: bwd(seq(steps=65)), "steps must be in [1, 64]"), (lambda: bwd(seq(steps=-1)), "steps must be in [1, 64]"),
             (lambda: fwd(seq(outer=0)), "outer and inner"), (lambda: bwd(seq(inner=0)), "outer and inner"), (lambda: fwd(seq(inner=-2)), "outer and inner"),
             (lambda: fwd(seq(stride0=-384)), "strides must be"), (lambda: bwd(seq(stride2=-128)), "strides must be"), (lambda: fwd(seq(stride2=130)), "strides must be"),
             (lambda: fwd(seq(h0=h0d.data_ptr() + 4)), "h0 must be"),
             (lambda: fwd(o=None), "out and h_last"), (lambda: fwd(h=hl.data_ptr() + 4), "out and h_last"), (lambda: fwd(hh=hist.data_ptr() + 8), "h_hist must be"),
             (lambda: fwd(w=ws.data_ptr() + 16), "workspace must be"),
             (lambda: bwd(hh=None), "h_hist is required"), (lambda: bwd(d=None), "h_hist, dout and dx"), (lambda: bwd(x_=dx.data_ptr() + 4), "h_hist, dout and dx"),
             (lambda: bwd(dl=dhd.data_ptr() + 4), "dh_last and dh0"), (lambda: bwd(d0=dh0.data_ptr() + 4), "dh_last and dh0"),
             (lambda: bwd(w=None), "workspace must be"), (lambda: bwd(w=ws.data_ptr() + 16), "workspace must be"), (lambda: bwd(wb=nb - 1), "workspace too small")]
    for i, (call, text) in enumerate(cases):
        assert call() == abi.HNS_ERR_INVALID_ARG, (i, text)
        assert text in lib.hns_last_error().decode(), (i, text, lib.hns_last_error().decode())
    torch.cuda.synchronize()
    for t in (out, hl, hist, dx, dh0, flat):
        assert bool((t == CANARY).all())                        # nothing was launched
    # the optional pointers: no h_hist forward; no dh_last and no dh0 backward
    assert fwd(hh=None) == abi.HNS_OK and fwd() == abi.HNS_OK and bwd(dl=None, d0=None) == abi.HNS_OK
    torch.cuda.synchronize()
    assert bool((out[:S * L * H] != CANARY).all()) and bool((out[S * L * H:] == CANARY).all()) and bool((dh0 == CANARY).all())
    assert bool(torch.isfinite(flat).all()) and bool((flat != CANARY).all()) and bool((dx[:S * L * H] != CANARY).all())


def test_report_ratios():
    print("gru gate ratios (worst):", {k: round(v, 2) for k, v in RATIOS.items()})
