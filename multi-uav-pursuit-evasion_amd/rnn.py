"""The reference's recurrent block as a differentiable op: HIP forward and backpropagation through time under torch.autograd.

`actor.rnn` / `critic.rnn` (learning/mappo.py, modules/rnn.py::GRU) put a GRU behind the encoder: an nn.GRUCell stepped over the sequence in a
Python loop, the carried state multiplied by 1 - is_init before every step, LayerNorm(output + input) behind it.  The fused updates refuse
that configuration; `gru` is the block alone — `hns_gru_forward` / `hns_gru_backward`, input size = hidden size = 128 — so a recurrent policy
is written in torch over `encoder.encode` -> `gru` -> a head (examples/recurrent_critic.py).  Collection calls it one step at a time
(`[S, 128]`, state in, state out); training re-runs the stored sequences (`[S, L, 128]`, or the encoder's `[B L A, 128]` features read in
place as `[B, A, L, 128]`), and one call over L steps gives the bits of L chained one-step calls.

The autograd node saves its inputs and the hidden states h_t ([S, L, 128]: the one activation; the gates are recomputed), is once
differentiable, writes the six parameter gradients into ONE flat allocation whose views it returns, and gives dx (with x's strides: the
encoder op's d features, no permute copy) and dh0.  `GRU` is the nn.Module form with the parameters under the reference's names.

CPU tensors run the torch restatement through the same node — forward without a graph, backward by autograd over the recomputed
restatement — so both devices have the same semantics (tests — not the hot path)."""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import abi
from . import policy as P

H = abi.HNS_GRU_HIDDEN
FIELDS = tuple(abi.GRU_NET_FIELDS)
# the reference's parameter names (modules/rnn.py: self.cell = nn.GRUCell, self.layer_norm = nn.LayerNorm) -> hns_gru_net fields
NAMES = {"cell.weight_ih": "weight_ih", "cell.weight_hh": "weight_hh", "cell.bias_ih": "bias_ih", "cell.bias_hh": "bias_hh",
         "layer_norm.weight": "ln_w", "layer_norm.bias": "ln_b"}
_SHAPES = {"weight_ih": (3 * H, H), "weight_hh": (3 * H, H), "bias_ih": (3 * H,), "bias_hh": (3 * H,), "ln_w": (H,), "ln_b": (H,)}
_N_FIXED = 4                                                   # _Gru.apply's arguments in front of the parameter tensors


def gru_parameters(params, stacked=False):
    """The six tensors by hns_gru_net field in FIELDS' order from a mapping of field names, checked: all present, fp32, contiguous, of the
    GRU's shapes.  stacked (one GRU per agent: DESIGN.md §7.18): every tensor [A, ...] with one A in [1, HNS_MAX_AGENTS]."""
    if not hasattr(params, "items"):
        raise TypeError(f"params must map hns_gru_net field names to tensors, not {type(params).__name__}")
    unknown = sorted(k for k in params if k not in FIELDS)
    if unknown:
        raise ValueError(f"gru: fields this network does not have: {unknown[:6]} (fields: {FIELDS})")
    missing = [f for f in FIELDS if f not in params]
    if missing:
        raise ValueError(f"gru: missing parameters {missing}")
    p = {f: params[f] for f in FIELDS}
    for f, t in p.items():
        if not torch.is_tensor(t):
            raise TypeError(f"gru parameter {f} must be a tensor, not {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"gru parameter {f} must be float32, not {t.dtype}")
        if tuple(t.shape[1:] if stacked else t.shape) != _SHAPES[f] or (stacked and t.dim() != len(_SHAPES[f]) + 1):
            raise ValueError(f"gru parameter {f} must be {('A',) + _SHAPES[f] if stacked else _SHAPES[f]}, not {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"gru parameter {f} must be contiguous")
    if stacked and (len({t.shape[0] for t in p.values()}) != 1 or not 1 <= p[FIELDS[0]].shape[0] <= abi.HNS_MAX_AGENTS):
        raise ValueError(f"stacked gru parameters need one leading agent dimension in [1, {abi.HNS_MAX_AGENTS}], not {sorted({t.shape[0] for t in p.values()})}")
    return p


def stacked_agents(p):
    """A of a stacked GRU (one per agent: weight_ih [A, 384, 128]); None for a single one."""
    return p["weight_ih"].shape[0] if p["weight_ih"].dim() == 3 else None


def restatement(p, x, h0, is_init):
    """include/hns.h's statements in torch: x [S, L, 128], h0 [S, 128], is_init [S, L] (0 / 1, x's dtype) -> (out [S, L, 128], h_last [S, 128])."""
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


def _net(p, grads=None):
    n = abi.HnsGruNet()
    for f, t in p.items():
        setattr(n, f, (grads[f] if grads is not None else t).data_ptr())
    return n


def _seq(x4, h0, init):
    s = abi.HnsGruSeq()
    B, A, L, _ = x4.shape
    for t, what, n in ((h0, "h0 [S, 128]", B * A * H), (init, "is_init [S, L]", B * A * L)):   # the kernels index them as declared: no strides travel
        if t is not None and (not t.is_contiguous() or t.numel() != n):
            raise ValueError(f"{what} must be contiguous and hold S = {B * A} sequences")
    s.x = x4.data_ptr()
    for d in range(3):
        s.x_stride[d] = x4.stride(d) if x4.shape[d] > 1 else 0
    s.outer, s.inner, s.steps = B, A, L
    s.h0 = h0.data_ptr() if h0 is not None else None
    s.is_init = init.data_ptr() if init is not None else None
    return s


def grad_layout(agents=None):
    """(offsets by field, floats) of the flat gradient allocation: FIELDS' order (every size is a multiple of four floats).  agents: A of a
    stacked GRU — every tensor A times the size, in the same order."""
    offsets, n = {}, 0
    for f in FIELDS:
        offsets[f] = n
        n += (agents or 1) * _SHAPES[f][0] * (_SHAPES[f][1] if len(_SHAPES[f]) > 1 else 1)
    return offsets, n


def _views(flat, agents=None):
    offsets, _ = grad_layout(agents)
    lead = (agents,) if agents else ()
    return {f: flat[offsets[f]:offsets[f] + torch.Size(lead + _SHAPES[f]).numel()].view(lead + _SHAPES[f]) for f in FIELDS}


def _agents_of(p, x4):
    """A of stacked parameters, checked against x4's agent dimension; None for a single GRU."""
    agents = stacked_agents(p)
    if agents is not None and agents != x4.shape[1]:
        raise ValueError(f"x has {x4.shape[1]} agents (dimension 1), the stacked GRU {agents}")
    return agents


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _buffer(t, shape, what, dev, strides=None):
    """The caller's buffer for `what`, checked: fp32 on `dev`, 16-byte aligned, of `shape` (contiguous, or with `strides`)."""
    want = tuple(strides) if strides is not None else None
    ok = torch.is_tensor(t) and t.dtype == torch.float32 and t.device == dev and tuple(t.shape) == tuple(shape) and t.data_ptr() % 16 == 0
    if ok and want is not None:
        ok = all(t.shape[d] == 1 or t.stride(d) == want[d] for d in range(t.dim()))
    elif ok:
        ok = t.is_contiguous()
    if not ok:
        raise ValueError(f"{what} must be a 16-byte aligned float32 {tuple(shape)} tensor on {dev}" + (f" with strides {want}" if want else ", contiguous"))
    return t


def device_forward(p, x4, h0, init, keep, out=None, h_last=None, h_hist=None):
    """hns_gru_forward on validated device tensors: (out with x4's strides, h_last [S, 128], h_hist [S, L, 128] or None).  out, h_last,
    h_hist: the caller's buffers (of those shapes; out with x4's strides) instead of tensors allocated per call.  Stacked parameters
    ([A, ...]: one GRU per agent, sequence (b, a) on slice a) go to hns_gru_forward_agents."""
    lib = abi.load_library()
    B, A, L, _ = x4.shape
    entry = lib.hns_gru_forward if _agents_of(p, x4) is None else lib.hns_gru_forward_agents
    dev = x4.device
    for f, t in p.items():
        if t.data_ptr() % 16:
            raise ValueError(f"gru parameter {f} must be 16-byte aligned")
    out = _buffer(out, x4.shape, "out", dev, x4.stride()) if out is not None else torch.empty_strided(x4.shape, x4.stride(), dtype=torch.float32, device=dev)
    h_last = _buffer(h_last, (B * A, H), "h_last", dev) if h_last is not None else torch.empty(B * A, H, dtype=torch.float32, device=dev)
    if keep:
        hist = _buffer(h_hist, (B * A, L, H), "h_hist", dev) if h_hist is not None else torch.empty(B * A, L, H, dtype=torch.float32, device=dev)
    else:
        hist = None
    net, seq = _net(p), _seq(x4, h0, init)
    with torch.cuda.device(dev):
        rc = entry(C.byref(net), C.byref(seq), out.data_ptr(), h_last.data_ptr(), hist.data_ptr() if keep else None, None, 0, _stream(dev))
    abi.check(rc, entry.__name__)
    return out, h_last, hist


def device_backward(p, x4, h0, init, hist, dout, dh_last, want_dh0, workspace=None, flat=None, dx=None):
    """hns_gru_backward on validated device tensors: ({field: gradient} — views of one allocation, dx with x4's strides, dh0 or None).
    workspace: a uint8 device tensor of at least hns_gru_workspace_bytes(S, L, 1) bytes, 256-byte aligned; flat: the gradients' flat fp32
    allocation (grad_layout's floats, 16-byte aligned); dx: a buffer with x4's shape and strides — the caller's instead of per-call ones.
    Stacked parameters go to hns_gru_backward_agents: the workspace is hns_gru_agents_workspace_bytes(B, A, L, 1), the gradients [A, ...]
    in grad_layout(A)'s floats."""
    lib = abi.load_library()
    B, A, L, _ = x4.shape
    dev = x4.device
    agents = _agents_of(p, x4)
    entry = lib.hns_gru_backward if agents is None else lib.hns_gru_backward_agents
    nbytes = lib.hns_gru_workspace_bytes(B * A, L, 1) if agents is None else lib.hns_gru_agents_workspace_bytes(B, A, L, 1)
    if workspace is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        ws = workspace
        if not torch.is_tensor(ws) or ws.dtype != torch.uint8 or ws.device != dev or not ws.is_contiguous() or ws.numel() < nbytes or ws.data_ptr() % 256:
            raise ValueError(f"workspace must be a contiguous, 256-byte aligned uint8 tensor of at least {nbytes} bytes on {dev}")
    n = grad_layout(agents)[1]
    if flat is None:
        flat = torch.empty(n, dtype=torch.float32, device=dev)
    elif (not torch.is_tensor(flat) or flat.dtype != torch.float32 or flat.device != dev or flat.dim() != 1 or flat.numel() < n or not flat.is_contiguous()
          or flat.data_ptr() % 16):
        raise ValueError(f"flat must be a contiguous 16-byte aligned float32 vector of at least {n} values on {dev}")
    grads = _views(flat, agents)
    dx = _buffer(dx, x4.shape, "dx", dev, x4.stride()) if dx is not None else torch.empty_strided(x4.shape, x4.stride(), dtype=torch.float32, device=dev)
    dh0 = torch.empty(B * A, H, dtype=torch.float32, device=dev) if want_dh0 else None
    net, grd, seq = _net(p), _net(p, grads), _seq(x4, h0, init)
    with torch.cuda.device(dev):
        rc = entry(C.byref(net), C.byref(seq), hist.data_ptr(), dout.data_ptr(), dh_last.data_ptr() if dh_last is not None else None,
                   C.byref(grd), dx.data_ptr(), dh0.data_ptr() if want_dh0 else None, ws.data_ptr(), nbytes, _stream(dev))
    abi.check(rc, entry.__name__)
    return grads, dx, dh0


def _cpu(p, x4, h0, init):
    B, A, L, _ = x4.shape
    x = x4.reshape(B * A, L, H)
    h = h0 if h0 is not None else x.new_zeros(B * A, H)
    m = init.to(x.dtype) if init is not None else x.new_zeros(B * A, L)
    out, h_last = restatement(p, x, h, m)
    return out.reshape(B, A, L, H), h_last


class _Gru(torch.autograd.Function):
    """gru's node.  Saved: its tensor inputs and the hidden states (nothing when no gradient will be asked for); the gates are recomputed."""

    @staticmethod
    def forward(ctx, x4, h0, init, save, *tensors):
        p = dict(zip(FIELDS, tensors))
        if x4.is_cuda:
            out, h_last, hist = device_forward(p, x4, h0, init, save)
        else:
            out, h_last = _cpu(p, x4, h0, init)
            hist = None
        if save:
            ctx.save_for_backward(x4, h0, init, hist, *tensors)
        return out, h_last

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, dh_last):
        x4, h0, init, hist, *tensors = ctx.saved_tensors
        p = dict(zip(FIELDS, tensors))
        need = ctx.needs_input_grad
        if x4.is_cuda:
            if dout.stride() != x4.stride():
                dout = torch.empty_strided(x4.shape, x4.stride(), dtype=torch.float32, device=x4.device).copy_(dout)
            elif dout.data_ptr() % 16:
                dout = dout.clone(memory_format=torch.preserve_format)
            dh_last = dh_last.contiguous()
            if dh_last.data_ptr() % 16:
                dh_last = dh_last.clone()
            grads, dx, dh0 = device_backward(p, x4, h0, init, hist, dout, dh_last, h0 is not None and need[1])
        else:
            leaves = {f: t.detach().requires_grad_(True) for f, t in p.items()}
            xl = x4.detach().requires_grad_(True)
            hl = h0.detach().requires_grad_(True) if h0 is not None else None
            with torch.enable_grad():
                out, h_last = _cpu(leaves, xl, hl, init)
                got = torch.autograd.grad([out, h_last], [xl] + ([hl] if hl is not None else []) + list(leaves.values()), [dout, dh_last])
            dx, dh0 = got[0], (got[1] if hl is not None else None)
            grads = _views(torch.empty(grad_layout()[1], dtype=torch.float32))
            for f, g in zip(FIELDS, got[-len(FIELDS):]):
                grads[f].copy_(g)
        return (dx if need[0] else None, dh0 if need[1] else None, None, None) + tuple(grads[f] if n else None for f, n in zip(FIELDS, need[_N_FIXED:]))


def _in_place(x4):
    """True iff the kernels can read x4 (and write out / dx with its strides) as it lies: the 128 values contiguous, 16-byte aligned rows,
    strides that keep the rows apart."""
    if x4.stride(3) != 1 or x4.data_ptr() % 16:
        return False
    dims = sorted(((x4.stride(d), x4.shape[d]) for d in range(3) if x4.shape[d] > 1))
    span = H
    for stride, size in dims:
        if stride < span or stride % 4:
            return False
        span = stride * size
    return True


def gru(params, x, h0=None, is_init=None):
    """(out, h_last) of the reference's GRU block: out_t = LayerNorm(h_t + x_t) with x's shape, h_last the state after the last step.

    params: a mapping of hns_gru_net field names (`FIELDS`; `GRU.parameters_by_field()`) to fp32 tensors.  x: fp32 `[S, L, 128]`,
    `[B, A, L, 128]` (sequence s = b A + a; any strides on the leading dimensions that keep the 128-value rows apart — the encoder op's
    `[B L A, 128]` features viewed as `[B, L, A, 128].transpose(1, 2)` are read in place) or `[S, 128]` (one step: collection), L <= 64.
    h0: `[S, 128]` / `[B, A, 128]` or None (zeros).  is_init: bool or 0 / 1 flags, `[S, L]` / `[B, A, L]` (a trailing 1 allowed), or
    `[B, 1, L]` for an env-level flag; None: none.  h_last: `[S, 128]` / `[B, A, 128]`.

    Gradients reach x (dx has x's strides), h0 and the parameters that require them; backward is once differentiable.  Under no_grad, or
    when nothing requires grad, nothing is saved and the hidden states are not written."""
    p = gru_parameters(params)
    if not torch.is_tensor(x):
        raise TypeError(f"x must be a tensor, not {type(x).__name__}")
    if x.dtype != torch.float32:
        raise TypeError(f"x must be float32, not {x.dtype}")
    if x.dim() not in (2, 3, 4) or x.shape[-1] != H:
        raise ValueError(f"x must be [S, {H}], [S, L, {H}] or [B, A, L, {H}], not {tuple(x.shape)}")
    lead = tuple(x.shape[:-2]) if x.dim() > 2 else tuple(x.shape[:1])
    x4 = x.unsqueeze(1).unsqueeze(1) if x.dim() == 2 else (x.unsqueeze(1) if x.dim() == 3 else x)
    B, A, L, _ = x4.shape
    S = B * A
    if S < 1:
        raise ValueError(f"x has no sequences: {tuple(x.shape)}")
    if not 1 <= L <= abi.HNS_GRU_MAX_STEPS:
        raise ValueError(f"the sequence length must be in [1, {abi.HNS_GRU_MAX_STEPS}] (the reference asserts train_seq_len <= train_every), not {L}")
    for f, t in p.items():
        if t.device != x.device:
            raise ValueError(f"gru parameter {f} is on {t.device}, x on {x.device}: all tensors must share one device")
    if h0 is not None:
        if not torch.is_tensor(h0) or h0.dtype != torch.float32:
            raise TypeError("h0 must be a float32 tensor")
        if h0.device != x.device:
            raise ValueError(f"h0 is on {h0.device}, x on {x.device}: all tensors must share one device")
        if tuple(h0.shape) != lead + (H,) and tuple(h0.shape) != (S, H):
            raise ValueError(f"h0 must be {lead + (H,)}, not {tuple(h0.shape)}")
        h0 = h0.reshape(S, H).contiguous()
        if h0.data_ptr() % 16:
            h0 = h0.clone()
    init = None
    if is_init is not None:
        if not torch.is_tensor(is_init):
            raise TypeError(f"is_init must be a tensor, not {type(is_init).__name__}")
        if is_init.device != x.device:
            raise ValueError(f"is_init is on {is_init.device}, x on {x.device}: all tensors must share one device")
        f = is_init != 0
        if f.numel() == S * L:
            f = f.reshape(S, L)
        elif x.dim() == 4 and f.dim() == 3 and tuple(f.shape) == (B, 1, L):
            f = f.expand(B, A, L).reshape(S, L)
        else:
            raise ValueError(f"is_init must have {S} x {L} flags (or be [B, 1, L] for a [B, A, L, {H}] input), not {tuple(is_init.shape)}")
        init = f.to(torch.uint8).contiguous()
    if x4.is_cuda and not _in_place(x4):
        x4 = x4.contiguous()
    save = torch.is_grad_enabled() and (x.requires_grad or (h0 is not None and h0.requires_grad) or any(t.requires_grad for t in p.values()))
    out, h_last = _Gru.apply(x4, h0, init, save, *p.values())
    out = out[:, 0, 0] if x.dim() == 2 else (out[:, 0] if x.dim() == 3 else out)
    return out, h_last.view(lead + (H,))


class GRU(nn.Module):
    """The reference's modules/rnn.py::GRU (input size = hidden size = 128) with `gru` as its forward pass.  The parameters sit under the
    reference's names (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh, layer_norm.weight, layer_norm.bias), initialised as the
    reference initialises them (nn.GRUCell's uniform biases, orthogonal weights), so `load_state_dict(reference_gru.state_dict())` works and
    the other way round.  `forward(input, h, is_initial)` has the reference's call shape and returns (output, h) with h padded to the
    sequence length as the reference pads it."""

    def __init__(self, input_size=H, hidden_size=H):
        super().__init__()
        if int(input_size) != H or int(hidden_size) != H:
            raise ValueError(f"the device GRU has input size = hidden size = {H} (the encoder's features), not {input_size} -> {hidden_size}")
        self.cell = nn.GRUCell(input_size=H, hidden_size=H)
        nn.init.orthogonal_(self.cell.weight_hh)
        nn.init.orthogonal_(self.cell.weight_ih)
        self.layer_norm = nn.LayerNorm(H)

    @classmethod
    def from_reference(cls, source, prefix="rnn."):
        """From an nn.Module, a TensorDict, a state_dict or a `MAPPOPolicy.state_dict()` checkpoint (its "actor_params" entry; pass the
        "critic" entry itself for a critic's): the six tensors under `prefix` (TensorDictModule's `module.` dropped), copied."""
        if isinstance(source, dict) and "actor_params" in source and "critic" in source:
            source = source["actor_params"]
        flat = {P._strip(k): v for k, v in P._flatten(source).items()}
        sd = {k[len(prefix):]: v.detach() for k, v in flat.items() if k.startswith(prefix) and k[len(prefix):] in NAMES}
        if set(sd) != set(NAMES):
            raise P.PolicyConfigError(f"no GRU under {prefix!r} (missing {sorted(set(NAMES) - set(sd))}; names: {sorted(flat)[:4]})")
        if sd["cell.weight_ih"].dim() != 2 or tuple(sd["cell.weight_ih"].shape) != (3 * H, H) or tuple(sd["cell.weight_hh"].shape) != (3 * H, H):
            raise P.PolicyConfigError(f"the GRU under {prefix!r} is not GRUCell({H}, {H}): weight_ih {tuple(sd['cell.weight_ih'].shape)}")
        mod = cls()
        mod.load_state_dict(sd)
        return mod.to(sd["cell.weight_ih"].device)

    def parameters_by_field(self):
        """{hns_gru_net field: parameter}: gru's `params`."""
        named = dict(self.named_parameters())
        return {f: named[k] for k, f in NAMES.items()}

    def forward(self, input, h=None, is_initial=None):
        has_time = input.dim() > 2
        if h is not None and has_time and h.dim() == input.dim():
            h = h.select(-2, 0)                                 # the reference's padded state: [N, L, H] -> its first step's
        out, h_last = gru(self.parameters_by_field(), input, h, is_initial)
        if has_time:
            h_last = h_last.unsqueeze(-2).expand(*input.shape[:-1], H)
        return out, h_last
