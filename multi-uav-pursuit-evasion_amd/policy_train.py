"""What the MAPPO critic's and actor's updates share on the host side of csrc/hns_policy_train.hip: the checks of a minibatch read in place from
the rollout, the preparation of a `hns_*_train_grad` call, the training restatement of the encoder, and the tail of every `update_*` — the
shared, the per-agent and the recurrent ones (`check_optimizer` before anything is launched, `clipped_step` behind the gradient call).

`critic_train` and `actor_train` keep what is their own — the reference's loss statements, their C call, their part of the cfg — and
`learner` drives both.  `validate` and `prepare_call` take the network's word ("critic" / "actor") and its per-row tensors, so a refusal
reads the same whichever update raised it.

`ClippedAdam` (optim's, re-exported here) is clip_grad_norm_ + torch.optim.Adam (amsgrad off, weight decay 0) with the device step every update
shares.  Every step bumps the parameters' version counters, so `policy.DevicePolicy` re-packs its operand image before the next forward pass.

`GradBucket` is the data-parallel caller's part (learner.DeviceLearner(group=)): one flat buffer behind a network's `.grad`
tensors, so the `*_train_grad_global` entries write straight into what ONE all-reduce sums and ONE `hns_grad_norm` call measures, between the
gradient call and the step.  DESIGN.md §7.4-7.5."""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import abi
from . import policy as P
from . import sharding
from .optim import ClippedAdam  # noqa: F401  (the two updates' optimiser, public here)


getter = P.getter


def check_optimizer(optimizer, caller, maker, cfg_check=None, cfg=None):
    """The refusals every update_* raises about its optimiser before anything is launched, in their order: not a ClippedAdam (TypeError
    naming `caller` and its `maker`), then `cfg_check(cfg)`'s — the caller's part of the algo cfg, whose result is returned — then a
    parameter group with weight_decay."""
    if not isinstance(optimizer, ClippedAdam):
        raise TypeError(f"{caller} takes a ClippedAdam ({maker}), not {type(optimizer).__name__}: the clip and the step are one launch that "
                        "needs the gradient norm")
    checked = cfg_check(cfg) if cfg_check is not None else None
    for pg in optimizer.param_groups:
        if pg.get("weight_decay", 0) != 0:
            raise NotImplementedError("weight_decay != 0 is not supported")
    return checked


def clipped_step(optimizer, grad_norm):
    """The tail of every update_*: clip_grad_norm_ + Adam on `grad_norm` (the loss-and-gradient call's); returns the norm to report."""
    optimizer.step(grad_norm=grad_norm)
    return optimizer.last_grad_norm if getattr(optimizer, "last_grad_norm", None) is not None else grad_norm


def check_workspace(workspace, nbytes, dev):
    """The caller's workspace (a uint8 device tensor of at least `nbytes` bytes, 256-byte aligned) as the kernels take it."""
    if not torch.is_tensor(workspace) or workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError(f"workspace must be a contiguous uint8 tensor on {dev}")
    if workspace.numel() < nbytes:
        raise ValueError(f"workspace holds {workspace.numel()} bytes, the minibatch needs {nbytes}")
    if workspace.data_ptr() % 256:
        raise ValueError("workspace must be 256-byte aligned")
    return workspace


def check_out(out, n, dev):
    """The caller's `n` fp32 result slots (a view into a table row) as the kernels write them."""
    if not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != dev or out.dim() != 1 or out.numel() != n or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 tensor of {n} values on {dev}")
    return out


def as_rollout(obs_self, obs_others, obs_cylinders):
    """The observations as [N, T, A, ...] views (a flat [R, A, ...] batch is [R, 1, A, ...]) — never a copy."""
    xs = obs_self
    if xs.dim() == obs_cylinders.dim() and xs.dim() in (4, 5) and xs.shape[-2] == 1:
        xs = xs.squeeze(-2)                                          # [.., A, 1, D] as the env writes state_self
    if xs.dim() == 3:
        xs = xs.unsqueeze(1)
        obs_others = obs_others.unsqueeze(1) if obs_others is not None else None
        obs_cylinders = obs_cylinders.unsqueeze(1)
    if xs.dim() != 4:
        raise ValueError(f"state_self must be [N, T, A, D] or [R, A, D] (optionally with a 1 before D), not {tuple(obs_self.shape)}")
    return xs, obs_others, obs_cylinders


def validate(word, p, xs, xo, xc, per_row, index, check_index):
    """Every refusal of hns_critic_train_grad / hns_actor_train_grad, raised here before anything is launched.  word: "critic" / "actor";
    per_row: (name, tensor, values per agent row) of the update's own [N T, A(, values)] tensors, in the order they are named."""
    for k, t in p.items():
        if not t.is_contiguous():
            raise ValueError(f"{word} parameter {k} must be contiguous")
    D = int(p["embed_self_w"].shape[1])
    N, T, A, Dx = xs.shape
    if Dx != D:
        raise ValueError(f"state_self rows have {Dx} values, the {word} takes {D}")
    if not 1 <= A <= abi.HNS_MAX_AGENTS:
        raise ValueError(f"{A} agents outside [1, {abi.HNS_MAX_AGENTS}]")
    has_others = "embed_others_w" in p
    if (xo is not None) != has_others or (A > 1) != has_others:
        raise ValueError(f"{A} agents: state_others is {'required' if A > 1 else 'absent'} for this network")
    if xo is not None and tuple(xo.shape) != (N, T, A, A - 1, 3):
        raise ValueError(f"state_others must be [{N}, {T}, {A}, {A - 1}, 3], not {tuple(xo.shape)}")
    if xc.dim() != 5 or tuple(xc.shape[:3]) != (N, T, A) or xc.shape[-1] != 5 or not 1 <= xc.shape[3] <= abi.HNS_MAX_CYLINDERS:
        raise ValueError(f"cylinders must be [{N}, {T}, {A}, K, 5] with K in [1, {abi.HNS_MAX_CYLINDERS}], not {tuple(xc.shape)}")
    for name, t in (("state_self", xs), ("state_others", xo), ("cylinders", xc), *((name, t) for name, t, _ in per_row)):
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, not {t.dtype}")
    steps = N * T
    if steps == 0:
        raise ValueError("the rollout holds no env-step")
    for name, t, width in per_row:
        if width == 1:
            if t.numel() != steps * A:
                raise ValueError(f"{name} must hold [N * T, A] = [{steps}, {A}] values, not {tuple(t.shape)}")
        elif t.numel() != steps * A * width or t.shape[-1] != width:
            raise ValueError(f"{name} must hold [N * T, A, {width}] = [{steps}, {A}, {width}] values, not {tuple(t.shape)}")
    if index is not None:
        if index.dtype != torch.int64 or index.dim() != 1:
            raise TypeError("index must be a 1-d int64 tensor")
        if index.numel() < 1:
            raise ValueError("empty minibatch: the mean over zero rows is NaN")
        if not index.is_contiguous():
            raise ValueError("index must be contiguous (the kernel reads it in place as consecutive int64): pass index.contiguous()")
        if check_index and not (xs.is_cuda and torch.cuda.is_current_stream_capturing()):
            lo, hi = torch.stack([index.min(), index.max()]).tolist()     # one host synchronisation
            if lo < 0 or hi >= steps:
                raise IndexError(f"index values [{lo}, {hi}] outside the {steps} env-steps of the rollout")
    devs = {t.device for t in (*p.values(), xs, xc, *(t for _, t, _ in per_row))} | ({xo.device} if xo is not None else set()) | \
        ({index.device} if index is not None else set())
    if len(devs) != 1:
        raise ValueError(f"parameters, observations, {', '.join(name for name, _, _ in per_row)} and index must share one device, not {devs}")
    return N, T, A, D, int(xc.shape[3])


def _batch(batch_type, xs, xo, xc, index, N, T, B):
    """The observation / index part of a `batch_type` (hns_critic_batch / hns_actor_batch) over tensors whose last stride is 1."""
    b = batch_type()
    b.obs_self, b.obs_cylinders = xs.data_ptr(), xc.data_ptr()
    b.obs_others = xo.data_ptr() if xo is not None else None
    b.self_stride[:] = [xs.stride(0), xs.stride(1), xs.stride(2)]
    b.others_stride[:] = [xo.stride(0), xo.stride(1), xo.stride(2), xo.stride(3)] if xo is not None else [0, 0, 0, 0]
    b.cyl_stride[:] = [xc.stride(0), xc.stride(1), xc.stride(2), xc.stride(3)]
    b.num_envs, b.num_steps, b.batch = N, T, B
    b.index = index.data_ptr() if index is not None else None
    b._keep = (xs, xo, xc)                                       # a fix-up copy lives as long as the struct that points at it
    return b


def fill_batch(batch_type, xs, xo, xc, index, shape):
    """`_batch` for a forward-only call (critic_train.value_loss_sums) on validated tensors; the per-row pointers are the caller's."""
    N, T = shape[:2]
    xs, xc = (t if t.stride(-1) == 1 else t.contiguous() for t in (xs, xc))
    if xo is not None and xo.stride(-1) != 1:
        xo = xo.contiguous()
    return _batch(batch_type, xs, xo, xc, index, N, T, index.numel() if index is not None else N * T)


def prepare_call(word, p, xs, xo, xc, index, shape, workspace_bytes, workspace, out, n_out, batch_type):
    """The arguments of a hns_*_train_grad call on validated device tensors: (net, grd, batch, ws, nbytes, scal, B, stream) — the filled
    hns_policy_net of the parameters and of their .grad tensors (created where absent), a `batch_type` with its observation / index part
    filled (the per-row pointers are the caller's), the workspace and its size by `workspace_bytes`, the `n_out` fp32 result slots, the
    env-steps of the minibatch and the current stream.  Every refusal comes first: nothing is allocated for a call that is refused."""
    N, T, A, D, K = shape
    dev = xs.device
    xs, xc = (t if t.stride(-1) == 1 else t.contiguous() for t in (xs, xc))
    if xo is not None and xo.stride(-1) != 1:
        xo = xo.contiguous()
    B = index.numel() if index is not None else N * T
    for f, t in p.items():
        if t.data_ptr() % 16:
            raise ValueError(f"{word} parameter {f} must be 16-byte aligned")
        if t.grad is not None and (t.grad.dtype != torch.float32 or not t.grad.is_contiguous() or t.grad.shape != t.shape or t.grad.device != dev):
            raise ValueError("existing .grad tensors must be contiguous float32 of the parameter's shape on its device")
    nbytes = workspace_bytes(B * A, D, A, K)
    if nbytes == 0:
        raise ValueError(f"shape outside the kernel's limits: {B * A} rows, self_dim {D}, {A} agents, {K} cylinders")
    ws = check_workspace(workspace, nbytes, dev) if workspace is not None else None
    scal = check_out(out, n_out, dev) if out is not None else None
    net, grd = abi.HnsPolicyNet(), abi.HnsPolicyNet()
    for f, t in p.items():
        if t.grad is None:
            t.grad = torch.empty_like(t)
        setattr(net, f, t.data_ptr())
        setattr(grd, f, t.grad.data_ptr())
    b = _batch(batch_type, xs, xo, xc, index, N, T, B)
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if scal is None:
        scal = torch.empty(n_out, dtype=torch.float32, device=dev)
    return net, grd, b, ws, nbytes, scal, B, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class GradBucket:
    """One flat fp32 buffer behind the `.grad` tensors of a network: every parameter's gradient is a contiguous view of `flat`, in the order
    given (registration order: the optimiser's), each view starting on a 16-byte boundary; the padding between them and behind the last one is
    zero and stays zero (nothing writes it), so it adds nothing to a sum or to the norm.  `prepare_call` and tp_train accept existing contiguous
    `.grad` tensors, so the device kernels write straight into the bucket.

    flat: the buffer ([numel padded to a multiple of 4]); all_reduce(group): SUM over the group, in place; norm(out=None): the 2-norm of
    `flat` as a one-element fp32 tensor (`out`: where to write it) — hns_grad_norm on the device, the fp64 sum of squares rounded once on the CPU;
    adopt(): after a CPU backward that REPLACED the `.grad` tensors, copies them into the views and puts the views back."""

    def __init__(self, parameters):
        self.params = list(parameters.values() if hasattr(parameters, "values") else parameters)
        if not self.params:
            raise ValueError("GradBucket needs at least one parameter")
        dev = self.params[0].device
        self.offsets, n = [], 0
        for p in self.params:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError("GradBucket takes float32 parameters on one device")
            self.offsets.append(n)
            n += (p.numel() + 3) // 4 * 4
        self.flat = torch.zeros(max(n, 4), dtype=torch.float32, device=dev)
        if self.flat.data_ptr() % 16:
            raise RuntimeError("the allocator returned a buffer that is not 16-byte aligned")
        self.views = [self.flat[o:o + p.numel()].view(p.shape) for o, p in zip(self.offsets, self.params)]
        for p, v in zip(self.params, self.views):
            p.grad = v
        self._ws = None

    def owns(self, parameters):
        """True when exactly these parameters, in this order, have their `.grad` in the bucket."""
        ps = list(parameters)
        return len(ps) == len(self.params) and all(a is b and a.grad is not None and a.grad.data_ptr() == v.data_ptr() and a.grad.shape == v.shape
                                                   for a, b, v in zip(ps, self.params, self.views))

    def adopt(self):
        with torch.no_grad():
            for p, v in zip(self.params, self.views):
                if p.grad is not v:
                    if p.grad is None:
                        v.zero_()
                    else:
                        v.copy_(p.grad)
                    p.grad = v

    def all_reduce(self, group):
        sharding.all_reduce_sum(self.flat, group)
        return self.flat

    def norm(self, out=None):
        dev = self.flat.device
        if out is None:
            out = torch.empty(1, dtype=torch.float32, device=dev)
        elif not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != dev or out.numel() != 1 or not out.is_contiguous():
            raise ValueError(f"out must be one float32 value on {dev}")
        if not self.flat.is_cuda:
            with torch.no_grad():
                out.copy_(self.flat.double().square().sum().sqrt().to(torch.float32).reshape(out.shape))
            return out
        lib = abi.load_library()
        n = self.flat.numel()
        nbytes = lib.hns_grad_norm_workspace_bytes(n)
        if self._ws is None:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = lib.hns_grad_norm(self.flat.data_ptr(), n, out.data_ptr(), self._ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        abi.check(rc, "hns_grad_norm")
        return out


def check_global(word, p, global_rows, rows, group, bucket):
    """The refusals of an update's data-parallel arguments: `global_rows` (all ranks' rows of the minibatch) covers this rank's; a `group`
    needs `global_rows` and a `bucket` that holds exactly this network's gradients."""
    if global_rows is None:
        if group is not None or bucket is not None:
            raise ValueError(f"{word}: group= and bucket= belong to the data-parallel call: pass global_rows= as well")
        return
    if int(global_rows) < rows:
        raise ValueError(f"{word}: global_rows {global_rows} is less than this rank's {rows} rows")
    if group is not None and bucket is None:
        raise ValueError(f"{word}: group= needs the GradBucket that is all-reduced (bucket=)")
    if bucket is not None and (len(bucket.params) != len(p) or any(a is not b for a, b in zip(bucket.params, p.values()))):
        raise ValueError(f"{word}: bucket= must be the GradBucket of this network's parameters, in their order")
    if bucket is not None and bucket.flat.is_cuda and not bucket.owns(p.values()):      # (a CPU backward replaces .grad; adopt() takes it in)
        raise ValueError(f"{word}: a parameter's .grad no longer lies in bucket=")


def finish_global(bucket, group, out=None):
    """What follows a `*_train_grad_global` call: the bucket's all-reduce over `group` (when given) and the norm of the result."""
    if bucket is None:
        return None
    if group is not None:
        bucket.all_reduce(group)
    return bucket.norm(out)


def encoder(p, xs, xo, xc):
    """PartialAttentionEncoder.forward as nn.MultiheadAttention(batch_first=True) runs it with key IS value (modules/networks.py:283-313):
    ONE transposed tensor serves as key and value, so torch projects k and v with one packed product — policy._encoder hands over two
    transposes, which gives the same forward bits but sums the token gradients in another order than the reference's backward."""
    E = P.EMBED_DIM
    toks = [F.linear(xs, p["embed_self_w"], p["embed_self_b"])]
    if xo is not None:
        toks.append(F.linear(xo, p["embed_others_w"], p["embed_others_b"]))
    toks.append(F.linear(xc, p["embed_cyl_w"], p["embed_cyl_b"]))
    x = F.layer_norm(torch.cat(toks, dim=-2), (E,), p["ln_w"], p["ln_b"])
    lead = x.shape[:-2]
    x = x.reshape(-1, x.shape[-2], E)
    res = x[:, [0]]                                              # (the reference's order of creation: autograd sums x's three uses in it)
    q, kv = x[:, [0]].transpose(1, 0), x.transpose(1, 0)
    attn = F.multi_head_attention_forward(q, kv, kv, E, 1, p["in_proj_w"], p["in_proj_b"], None, None, False, 0.0, p["out_proj_w"],
                                          p["out_proj_b"], training=True, need_weights=False)[0].transpose(1, 0)
    x = F.layer_norm(res + attn, (E,), p["norm1_w"], p["norm1_b"])
    x = F.layer_norm(x + F.linear(F.gelu(F.linear(x, p["linear1_w"], p["linear1_b"])), p["linear2_w"], p["linear2_b"]), (E,),
                     p["norm2_w"], p["norm2_b"])
    return x.mean(-2).reshape(*lead, E)
