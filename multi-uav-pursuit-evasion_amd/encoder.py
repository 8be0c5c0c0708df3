"""The PartialAttentionEncoder as a differentiable op: HIP forward and backward under torch.autograd.

The fused updates (`critic_train.update_critic`, `actor_train.update_actor`, `learner.DeviceLearner`) cover cfg/algo/mappo.yaml's defaults and
refuse everything else.  Nearly all of an update's cost is the encoder (modules/networks.py:250-313); the head and the loss are a few flops
per row.  `encode` is that encoder alone: the 128 features of every (env-step, agent) row forward (`hns_encoder_forward`), the gradients of
its 20 parameter tensors from d features backward (`hns_encoder_backward`), so any head, loss, optimiser or schedule — a TanhNormal head,
per-agent heads, an auxiliary loss, AdamW, StepLR — is plain torch on top of it.  examples/custom_head.py is one such configuration.

The backward kernel recomputes its tile's forward pass, so the autograd node keeps no activation: it saves its inputs alone (the version
check of `save_for_backward` then catches a parameter stepped between forward and backward), is once differentiable, and writes every
gradient into ONE flat allocation whose views it returns.  Observation gradients are not provided.

`AttentionEncoder` is the nn.Module form, with its parameters under the reference's names: `load_state_dict` takes a reference encoder's
`state_dict()` and the other way round.

CPU tensors run the torch restatement (`policy_train.encoder`) through the same node — forward without a graph, backward by autograd over
the recomputed restatement — so both devices have the same semantics (tests, gloo runs — not the hot path)."""
import ctypes as C

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import abi
from . import policy as P
from . import policy_train as PT

FIELDS = tuple(P._ENCODER.values())                            # the 20 tensors, in the reference's registration order
_HEAD = ("head_w", "head_b", "log_std")
_N_FIXED = 6                                                   # _Encode.apply's arguments in front of the parameter tensors


def _shapes(D):
    E = P.EMBED_DIM
    return {"embed_self_w": (E, D), "embed_self_b": (E,), "embed_others_w": (E, 3), "embed_others_b": (E,), "embed_cyl_w": (E, 5), "embed_cyl_b": (E,),
            "in_proj_w": (3 * E, E), "in_proj_b": (3 * E,), **{f: (E, E) for f in ("out_proj_w", "linear1_w", "linear2_w")},
            **{f: (E,) for f in ("ln_w", "ln_b", "out_proj_b", "linear1_b", "linear2_b", "norm1_w", "norm1_b", "norm2_w", "norm2_b")}}


def encoder_parameters(params, stacked=False):
    """The encoder's tensors by hns_policy_net field in FIELDS' order from a mapping of field names (a head's fields are ignored), checked:
    every tensor but the state_others embedding present, fp32, of the encoder's shapes.  stacked (one encoder per agent: DESIGN.md §7.18):
    every tensor [A, ...] with one A in [1, HNS_MAX_AGENTS], each slice of those shapes."""
    if not hasattr(params, "items"):
        raise TypeError(f"params must map hns_policy_net field names to tensors, not {type(params).__name__}")
    unknown = sorted(k for k in params if k not in FIELDS and k not in _HEAD)
    if unknown:
        raise ValueError(f"encoder: fields this network does not have: {unknown[:6]} (fields: policy._ENCODER's values)")
    p = {f: params[f] for f in FIELDS if f in params}
    missing = sorted(set(FIELDS) - set(p) - {"embed_others_w", "embed_others_b"})
    if missing or ("embed_others_w" in p) != ("embed_others_b" in p):
        raise ValueError(f"encoder: missing parameters {missing or ['embed_others_w / embed_others_b']}")
    for f, t in p.items():
        if not torch.is_tensor(t):
            raise TypeError(f"encoder parameter {f} must be a tensor, not {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"encoder parameter {f} must be float32, not {t.dtype}")
    sw = p["embed_self_w"]
    lead = 1 if stacked else 0
    if sw.dim() != 2 + lead or not 1 <= sw.shape[-1] <= abi.HNS_POLICY_MAX_SELF_DIM:
        raise ValueError(f"encoder: the state_self embedding must be Linear(D, 128) with D in [1, {abi.HNS_POLICY_MAX_SELF_DIM}]"
                         f"{' under a leading agent dimension' if stacked else ''}, not {tuple(sw.shape)}")
    want = _shapes(int(sw.shape[-1]))
    for f, t in p.items():
        if tuple(t.shape[lead:]) != want[f] or t.dim() != len(want[f]) + lead:
            raise ValueError(f"encoder parameter {f} must be {('A',) + want[f] if stacked else want[f]}, not {tuple(t.shape)}")
    if stacked:
        sizes = sorted({int(t.shape[0]) for t in p.values()})
        if len(sizes) != 1 or not 1 <= sizes[0] <= abi.HNS_MAX_AGENTS:
            raise ValueError(f"stacked encoder parameters need one leading agent dimension in [1, {abi.HNS_MAX_AGENTS}], not {sizes}")
        for f, t in p.items():
            if not t.is_contiguous():
                raise ValueError(f"stacked encoder parameter {f} must be contiguous")
    return p


def stacked_agents(p):
    """A of a stacked encoder (one per agent: in_proj_w [A, 384, 128]); None for a single one."""
    return int(p["in_proj_w"].shape[0]) if p["in_proj_w"].dim() == 3 else None


def _entries(p, shape, backward):
    """(the entry, its workspace query) for these parameters: the shared op's, or for stacked parameters the _agents forms'."""
    lib = abi.load_library()
    agents = stacked_agents(p)
    if agents is None:
        return (lib.hns_encoder_backward if backward else lib.hns_encoder_forward), lib.hns_encoder_workspace_bytes
    if agents != shape[2]:
        raise ValueError(f"the observation has {shape[2]} agents, the stacked encoder {agents}")
    return (lib.hns_encoder_backward_agents if backward else lib.hns_encoder_forward_agents), lib.hns_encoder_agents_workspace_bytes


def _gather(xs, xo, xc, index):
    N, T, A, D = xs.shape
    xs, xc = xs.reshape(N * T, A, 1, D), xc.reshape(N * T, A, xc.shape[3], 5)
    xo = xo.reshape(N * T, A, A - 1, 3) if xo is not None else None
    if index is not None:
        xs, xc = xs[index], xc[index]
        xo = xo[index] if xo is not None else None
    return xs, xo, xc


def _net(p, grads=None):
    n = abi.HnsPolicyNet()
    for f, t in p.items():
        setattr(n, f, (grads[f] if grads is not None else t).data_ptr())
    return n


def grad_layout(p):
    """(offsets by field, floats) of the flat gradient allocation: FIELDS' order, every tensor — stacked ones whole, [A, ...] — on a 16-byte
    boundary."""
    offsets, n = {}, 0
    for f, t in p.items():
        offsets[f] = n
        n += (t.numel() + 3) // 4 * 4
    return offsets, n


def device_forward(p, xs, xo, xc, index, shape, workspace=None, out=None):
    """hns_encoder_forward on validated device tensors: features [B, A, 128] (`out`: a contiguous fp32 tensor of that many values, written in
    place).  `workspace`: a uint8 device tensor of at least hns_encoder_workspace_bytes(rows, ..., 0) bytes, 256-byte aligned.  Stacked
    parameters ([A, ...]: one encoder per agent, row (b, a) on slice a) go to hns_encoder_forward_agents, with its workspace query."""
    entry, query = _entries(p, shape, False)
    N, T, A, D, K = shape
    dev = xs.device
    B = index.numel() if index is not None else N * T
    for f, t in p.items():
        if t.data_ptr() % 16:
            raise ValueError(f"encoder parameter {f} must be 16-byte aligned")
    nbytes = query(B * A, D, A, K, 0)
    if nbytes == 0:
        raise ValueError(f"shape outside the kernel's limits: {B * A} rows, self_dim {D}, {A} agents, {K} cylinders")
    ws = PT.check_workspace(workspace, nbytes, dev) if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    b = PT.fill_batch(abi.HnsCriticBatch, xs, xo, xc, index, shape)
    feats = out if out is not None else torch.empty(B, A, P.EMBED_DIM, dtype=torch.float32, device=dev)
    net = _net(p)
    with torch.cuda.device(dev):
        rc = entry(C.byref(net), C.byref(b), D, A, K, feats.data_ptr(), ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    abi.check(rc, entry.__name__)
    return feats


def device_backward(p, xs, xo, xc, index, shape, dfeatures, workspace=None, flat=None):
    """hns_encoder_backward on validated device tensors: ({field: gradient}, flat) — every gradient a view of the ONE allocation `flat`
    (grad_layout; `flat`: the caller's, at least that many fp32 values, 16-byte aligned).  dfeatures: contiguous fp32 [B, A, 128].  Stacked
    parameters go to hns_encoder_backward_agents: every gradient [A, ...], agent a's slice from its own rows."""
    entry, query = _entries(p, shape, True)
    N, T, A, D, K = shape
    dev = xs.device
    B = index.numel() if index is not None else N * T
    if dfeatures.dtype != torch.float32 or dfeatures.device != dev or dfeatures.numel() != B * A * P.EMBED_DIM or not dfeatures.is_contiguous():
        raise ValueError(f"d features must be contiguous float32 [{B}, {A}, {P.EMBED_DIM}] on {dev}")
    if dfeatures.data_ptr() % 16:
        dfeatures = dfeatures.clone()
    nbytes = query(B * A, D, A, K, 1)
    if nbytes == 0:
        raise ValueError(f"shape outside the kernel's limits: {B * A} rows, self_dim {D}, {A} agents, {K} cylinders")
    ws = PT.check_workspace(workspace, nbytes, dev) if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    offsets, n = grad_layout(p)
    if flat is None:
        flat = torch.empty(n, dtype=torch.float32, device=dev)
    elif flat.dtype != torch.float32 or flat.device != dev or flat.dim() != 1 or flat.numel() < n or not flat.is_contiguous() or flat.data_ptr() % 16:
        raise ValueError(f"flat must be a contiguous 16-byte aligned float32 vector of at least {n} values on {dev}")
    grads = {f: flat[offsets[f]:offsets[f] + t.numel()].view(t.shape) for f, t in p.items()}
    b = PT.fill_batch(abi.HnsCriticBatch, xs, xo, xc, index, shape)
    net, grd = _net(p), _net(p, grads)
    with torch.cuda.device(dev):
        rc = entry(C.byref(net), C.byref(b), D, A, K, dfeatures.data_ptr(), C.byref(grd), ws.data_ptr(), nbytes,
                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    abi.check(rc, entry.__name__)
    return grads, flat


class _Encode(torch.autograd.Function):
    """encode's node.  Saved: its tensor inputs alone (nothing when no gradient will be asked for); the forward pass is recomputed."""

    @staticmethod
    def forward(ctx, xs, xo, xc, index, aux, fields, *tensors):
        shape, workspace, save = aux
        p = dict(zip(fields, tensors))
        if xs.is_cuda:
            feats = device_forward(p, xs, xo, xc, index, shape, workspace)
        else:
            feats = PT.encoder(p, *_gather(xs, xo, xc, index))
        if save:
            ctx.save_for_backward(xs, xo, xc, index, *tensors)
            ctx.fields, ctx.shape, ctx.workspace = fields, shape, workspace
        return feats

    @staticmethod
    @once_differentiable
    def backward(ctx, dfeatures):
        xs, xo, xc, index, *tensors = ctx.saved_tensors
        need = ctx.needs_input_grad[_N_FIXED:]
        p = dict(zip(ctx.fields, tensors))
        dfeatures = dfeatures.contiguous()
        if xs.is_cuda:
            grads, _ = device_backward(p, xs, xo, xc, index, ctx.shape, dfeatures, ctx.workspace)
        else:
            offsets, n = grad_layout(p)
            flat = torch.empty(n, dtype=torch.float32)
            grads = {f: flat[offsets[f]:offsets[f] + t.numel()].view(t.shape) for f, t in p.items()}
            leaves = {f: t.detach().requires_grad_(True) for f, t in p.items()}
            with torch.enable_grad():
                feats = PT.encoder(leaves, *_gather(xs, xo, xc, index))
                got = torch.autograd.grad(feats, list(leaves.values()), dfeatures)
            for f, g in zip(leaves, got):
                grads[f].copy_(g)
        return (None,) * _N_FIXED + tuple(grads[f] if n else None for f, n in zip(ctx.fields, need))


def encode(params, obs_self, obs_others, obs_cylinders, index=None, workspace=None, check_index=True):
    """The encoder's features [B, A, 128] of a minibatch, differentiable with respect to the parameters.

    params: a mapping of hns_policy_net field names to fp32 tensors (policy._ENCODER's values; what policy.parse_parameters yields, the head's
    fields ignored).  obs_*: the rollout's [N, T, A, ...] observations with `index` (int64 [B] env-steps of the flattened [N T]; None: all), read
    in place as the updates read them, or a flat [S, A, ...] batch; state_others None with one agent.  Row (b, a) is env-step index[b], agent a.
    `check_index` range-checks the index (one host synchronisation).  `workspace`: a uint8 device tensor, 256-byte aligned, of at least
    hns_encoder_workspace_bytes(B A, D, A, K, 1) bytes (0 instead of 1 when no gradient is asked for) instead of one allocated per call; forward
    and backward both use it, each from scratch (nothing is kept in it between them).

    Gradients reach the parameters that require them; observations must not require grad (their gradients are not provided).  Backward is once
    differentiable.  Under no_grad, or when no parameter requires grad, nothing is saved."""
    p = encoder_parameters(params)
    for name, t in (("state_self", obs_self), ("state_others", obs_others), ("cylinders", obs_cylinders)):
        if t is not None and not torch.is_tensor(t):
            raise TypeError(f"{name} must be a tensor, not {type(t).__name__}")
        if t is not None and t.requires_grad:
            raise ValueError(f"{name} requires grad: observation gradients are not provided by the encoder op (detach the observations)")
    xs, xo, xc = PT.as_rollout(obs_self, obs_others, obs_cylinders)
    shape = PT.validate("encoder", p, xs, xo, xc, (), index, check_index)
    save = torch.is_grad_enabled() and any(t.requires_grad for t in p.values())
    if workspace is not None and xs.is_cuda:
        N, T, A, D, K = shape
        rows = (index.numel() if index is not None else N * T) * A
        PT.check_workspace(workspace, abi.load_library().hns_encoder_workspace_bytes(rows, D, A, K, 1 if save else 0), xs.device)
    return _Encode.apply(xs, xo, xc, index, (shape, workspace, save), tuple(p), *p.values())


class _Embed(nn.Module):
    def __init__(self, self_dim, others):
        super().__init__()
        E = P.EMBED_DIM
        keys = [("state_self", self_dim)] + ([("state_others", 3)] if others else []) + [("cylinders", 5)]
        self.embed = nn.ModuleDict({k: nn.Linear(i, E) for k, i in keys})
        self.layer_norm = nn.LayerNorm(E)


class AttentionEncoder(nn.Module):
    """The reference's PartialAttentionEncoder (embed_dim 128, one head, dim_feedforward 128) with `encode` as its forward pass.  The parameters
    sit under the reference's names (policy._ENCODER's keys: split_embed.embed.state_self.weight, attn.in_proj_weight, ...), so
    `load_state_dict(reference_encoder.state_dict())` works, and `state_dict()` loads into a reference encoder.

    AttentionEncoder(self_dim, num_agents): initialised as policy.random_parameters initialises an encoder (seed: its seed); one agent has no
    state_others embedding.  `from_reference(source, prefix)` reads an actor's ("encoder.") or a critic's ("base.") encoder."""

    def __init__(self, self_dim, num_agents, seed=0):
        super().__init__()
        E = P.EMBED_DIM
        if not 1 <= int(self_dim) <= abi.HNS_POLICY_MAX_SELF_DIM or not 1 <= int(num_agents) <= abi.HNS_MAX_AGENTS:
            raise ValueError(f"self_dim must be in [1, {abi.HNS_POLICY_MAX_SELF_DIM}] and num_agents in [1, {abi.HNS_MAX_AGENTS}]")
        self.self_dim, self.has_others = int(self_dim), int(num_agents) > 1
        self.split_embed = _Embed(self.self_dim, self.has_others)
        self.attn = nn.MultiheadAttention(E, 1, batch_first=True)
        self.linear1, self.linear2 = nn.Linear(E, E), nn.Linear(E, E)
        self.norm1, self.norm2 = nn.LayerNorm(E), nn.LayerNorm(E)
        actor, _ = P.random_parameters(self.self_dim, int(num_agents), seed)
        self.load_state_dict({k[len("encoder."):]: v for k, v in actor.items() if k.startswith("encoder.")})

    @classmethod
    def from_reference(cls, source, prefix="encoder."):
        """From an nn.Module, a TensorDict, a state_dict or a `MAPPOPolicy.state_dict()` checkpoint (its "actor_params" entry for "encoder.", its
        "critic" entry for "base."): the tensors under `prefix` (TensorDictModule's `module.` dropped), copied."""
        if isinstance(source, dict) and "actor_params" in source and "critic" in source:
            source = source["actor_params" if prefix == "encoder." else "critic"]
        flat = {P._strip(k): v for k, v in P._flatten(source).items()}
        sd = {k[len(prefix):]: v.detach() for k, v in flat.items() if k.startswith(prefix) and k[len(prefix):] in P._ENCODER}
        key = "split_embed.embed.state_self.weight"
        if key not in sd:
            raise P.PolicyConfigError(f"no PartialAttentionEncoder under {prefix!r} (names: {sorted(flat)[:4]})")
        if sd[key].dim() != 2:
            raise P.PolicyConfigError("parameters with a leading agent dimension (share_actor: False) hold one encoder per agent: pass one agent's slice")
        enc = cls(int(sd[key].shape[1]), 2 if "split_embed.embed.state_others.weight" in sd else 1)
        enc.load_state_dict(sd)
        return enc.to(sd[key].device)

    def parameters_by_field(self):
        """{hns_policy_net field: parameter}: encode's `params`."""
        named = dict(self.named_parameters())
        return {f: named[k] for k, f in P._ENCODER.items() if k in named}

    def forward(self, obs_self, obs_others, obs_cylinders, index=None, workspace=None, check_index=True):
        return encode(self.parameters_by_field(), obs_self, obs_others, obs_cylinders, index, workspace, check_index)
