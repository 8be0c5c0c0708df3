"""The MAPPO critic's update on the device: MAPPOPolicy.update_critic (learning/mappo.py:326-352) for make_critic's network at
cfg/algo/mappo.yaml's defaults (critic_input: obs, no rnn, weight_decay 0).

`value_loss_and_grad(critic, obs_self, obs_others, obs_cylinders, b_values, b_returns, index)` is update_critic up to `backward()`: device
tensors go to ONE call of `hns_critic_train_grad` (forward + loss partials, the branch decision of the max of the two mean losses, the
encoder's backward pass, the weight-gradient products, fixed-order sums) that fills every parameter's `.grad` in its PyTorch layout and
returns value_loss, explained_var and the total gradient norm as 0-dim device tensors — no autograd graph, no host synchronisation.  `index`
reads a minibatch of `make_dataset_naive` (mappo.py:493-513, seq_len 1) in place from the rollout's [N, T, A, ...] observations.

`ClippedAdam` is clip_grad_norm_ + torch.optim.Adam (amsgrad off, weight decay 0) in ONE launch of `hns_adam_clipped` over all tensors and a
device-resident step counter; its state_dict is Adam's, both ways.  Every step bumps the parameters' version counters, so
`policy.DevicePolicy` re-packs its operand image before the next forward pass.  A data-parallel caller all-reduces the `.grad` tensors and
recomputes the norm between the two calls.

`update_critic` is the reference's function.  CPU tensors run the reference's torch statements throughout (CPU tests, gloo runs — not the
hot path).  DESIGN.md §7.4."""
import collections
import ctypes as C
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import abi
from . import policy as P
from .tp_train import TPAdam

CriticLoss = collections.namedtuple("CriticLoss", ["value_loss", "explained_var", "grad_norm", "values"])
LOSSES = {"huber": abi.HNS_CRITIC_LOSS_HUBER, "mse": abi.HNS_CRITIC_LOSS_MSE}


def _check(rc, what):
    if rc != abi.HNS_OK:
        raise RuntimeError(f"{what} failed ({rc}): {abi.load_library().hns_last_error().decode()}")


def _getter(cfg):
    if cfg is None:
        return lambda k, d=None: d
    return cfg.get if hasattr(cfg, "get") else (lambda k, d=None: getattr(cfg, k, d))


def _check_workspace(workspace, nbytes, dev):
    """The caller's workspace (a uint8 device tensor of at least `nbytes` bytes, 256-byte aligned) as the kernels take it."""
    if not torch.is_tensor(workspace) or workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError(f"workspace must be a contiguous uint8 tensor on {dev}")
    if workspace.numel() < nbytes:
        raise ValueError(f"workspace holds {workspace.numel()} bytes, the minibatch needs {nbytes}")
    if workspace.data_ptr() % 256:
        raise ValueError("workspace must be 256-byte aligned")
    return workspace


def _check_out(out, n, dev):
    """The caller's `n` fp32 result slots (a view into a table row) as the kernels write them."""
    if not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != dev or out.dim() != 1 or out.numel() != n or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 tensor of {n} values on {dev}")
    return out


def critic_parameters(critic):
    """The critic's tensors by hns_policy_net field, in the order the module registers them (clip_grad_norm_'s order)."""
    return P.parse_parameters(critic, P.CRITIC_NAMES, "critic")


def _as_rollout(obs_self, obs_others, obs_cylinders):
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


def _validate(p, xs, xo, xc, b_values, b_returns, index, check_index):
    """Every refusal of hns_critic_train_grad, raised here before anything is launched."""
    for k, t in p.items():
        if not t.is_contiguous():
            raise ValueError(f"critic parameter {k} must be contiguous")
    D = int(p["embed_self_w"].shape[1])
    N, T, A, Dx = xs.shape
    if Dx != D:
        raise ValueError(f"state_self rows have {Dx} values, the critic takes {D}")
    if not 1 <= A <= abi.HNS_MAX_AGENTS:
        raise ValueError(f"{A} agents outside [1, {abi.HNS_MAX_AGENTS}]")
    has_others = "embed_others_w" in p
    if (xo is not None) != has_others or (A > 1) != has_others:
        raise ValueError(f"{A} agents: state_others is {'required' if A > 1 else 'absent'} for this network")
    if xo is not None and tuple(xo.shape) != (N, T, A, A - 1, 3):
        raise ValueError(f"state_others must be [{N}, {T}, {A}, {A - 1}, 3], not {tuple(xo.shape)}")
    if xc.dim() != 5 or tuple(xc.shape[:3]) != (N, T, A) or xc.shape[-1] != 5 or not 1 <= xc.shape[3] <= abi.HNS_MAX_CYLINDERS:
        raise ValueError(f"cylinders must be [{N}, {T}, {A}, K, 5] with K in [1, {abi.HNS_MAX_CYLINDERS}], not {tuple(xc.shape)}")
    for name, t in (("state_self", xs), ("state_others", xo), ("cylinders", xc), ("b_values", b_values), ("b_returns", b_returns)):
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, not {t.dtype}")
    steps = N * T
    if steps == 0:
        raise ValueError("the rollout holds no env-step")
    for name, t in (("b_values", b_values), ("b_returns", b_returns)):
        if t.numel() != steps * A:
            raise ValueError(f"{name} must hold [N * T, A] = [{steps}, {A}] values, not {tuple(t.shape)}")
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
    devs = {t.device for t in (*p.values(), xs, xc, b_values, b_returns)} | ({xo.device} if xo is not None else set()) | \
        ({index.device} if index is not None else set())
    if len(devs) != 1:
        raise ValueError(f"parameters, observations, b_values, b_returns and index must share one device, not {devs}")
    return N, T, A, D, int(xc.shape[3])


def _encoder(p, xs, xo, xc):
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


def _torch_loss_and_grad(p, xs, xo, xc, b_values, b_returns, index, clip_param, loss, huber_delta):
    """update_critic's statements (mappo.py:328-341) on the gathered minibatch; autograd through the encoder above."""
    N, T, A, D = xs.shape
    xs, xc = xs.reshape(N * T, A, 1, D), xc.reshape(N * T, A, xc.shape[3], 5)
    xo = xo.reshape(N * T, A, A - 1, 3) if xo is not None else None
    bv, ret = b_values.reshape(N * T, A, 1), b_returns.reshape(N * T, A, 1)
    if index is not None:
        xs, xc, bv, ret = xs[index], xc[index], bv[index], ret[index]
        xo = xo[index] if xo is not None else None
    leaves = {k: v.detach().requires_grad_(True) for k, v in p.items()}
    values = F.linear(_encoder(leaves, xs, xo, xc), leaves["head_w"], leaves["head_b"])
    clipped = bv + (values - bv).clamp(-clip_param, clip_param)
    loss_fn = nn.HuberLoss(delta=huber_delta) if loss == "huber" else nn.MSELoss()
    l_clip = loss_fn(ret, clipped)
    l_orig = loss_fn(ret, values)
    value_loss = torch.max(l_orig, l_clip)
    grads = torch.autograd.grad(value_loss, list(leaves.values()))
    for t, g in zip(p.values(), grads):
        t.grad = g
    with torch.no_grad():
        grad_norm = nn.utils.clip_grad_norm_(list(p.values()), float("inf"))      # the total norm as clip_grad_norm_ forms it; scales by 1
        explained_var = 1 - F.mse_loss(values, ret) / ret.var()
    return CriticLoss(value_loss.detach(), explained_var, grad_norm, values.detach())


def value_loss_and_grad(critic, obs_self, obs_others, obs_cylinders, b_values, b_returns, index=None, clip_param=0.1, loss="huber",
                        huber_delta=10.0, check_index=True, workspace=None, out=None):
    """The clipped value loss of the critic on a minibatch and every parameter's .grad (as zero_grad() + backward() leave them, before
    clip_grad_norm_).  Returns CriticLoss(value_loss, explained_var, grad_norm: 0-dim tensors; values [B, A, 1]).

    obs_*: the rollout's [N, T, A, ...] observations (state_self [N, T, A, D] or [N, T, A, 1, D]; state_others None with one agent) or a
    flat [R, A, ...] batch, read in place; b_values, b_returns: [N, T, A, 1] (any shape of N T A values); index: int64 [B] env-steps of the
    flattened [N T] (None: all).  `check_index` range-checks the index (one host synchronisation; skipped inside a graph capture).
    `workspace`: a uint8 device tensor of at least hns_critic_train_workspace_bytes bytes, 256-byte aligned, instead of one allocated per call;
    `out`: three fp32 device values that receive value_loss, explained_var and grad_norm (the returned scalars are views of it) instead of a
    tensor of the call's own.  Both are ignored on the CPU."""
    if loss not in LOSSES:
        raise ValueError(f"loss must be 'huber' or 'mse', not {loss!r}")
    if not clip_param >= 0 or (loss == "huber" and not huber_delta > 0):
        raise ValueError("clip_param must be >= 0 and huber_delta > 0")
    p = critic_parameters(critic)
    xs, xo, xc = _as_rollout(obs_self, obs_others, obs_cylinders)
    N, T, A, D, K = _validate(p, xs, xo, xc, b_values, b_returns, index, check_index)
    if not xs.is_cuda:
        return _torch_loss_and_grad(p, xs, xo, xc, b_values, b_returns, index, float(clip_param), loss, float(huber_delta))
    dev = xs.device
    lib = abi.load_library()
    xs, xc = (t if t.stride(-1) == 1 else t.contiguous() for t in (xs, xc))
    if xo is not None and xo.stride(-1) != 1:
        xo = xo.contiguous()
    bv, ret = b_values.contiguous(), b_returns.contiguous()
    B = index.numel() if index is not None else N * T
    net, grd = abi.HnsPolicyNet(), abi.HnsPolicyNet()
    for f, t in p.items():                                      # every refusal first: nothing is allocated for a call that is refused
        if t.data_ptr() % 16:
            raise ValueError(f"critic parameter {f} must be 16-byte aligned")
        if t.grad is not None and (t.grad.dtype != torch.float32 or not t.grad.is_contiguous() or t.grad.shape != t.shape or t.grad.device != dev):
            raise ValueError("existing .grad tensors must be contiguous float32 of the parameter's shape on its device")
    nbytes = lib.hns_critic_train_workspace_bytes(B * A, D, A, K)
    if nbytes == 0:
        raise ValueError(f"shape outside the kernel's limits: {B * A} rows, self_dim {D}, {A} agents, {K} cylinders")
    ws = _check_workspace(workspace, nbytes, dev) if workspace is not None else None
    scal = _check_out(out, 3, dev) if out is not None else None
    for f, t in p.items():
        if t.grad is None:
            t.grad = torch.empty_like(t)
        setattr(net, f, t.data_ptr())
        setattr(grd, f, t.grad.data_ptr())
    b = abi.HnsCriticBatch()
    b.obs_self, b.obs_cylinders = xs.data_ptr(), xc.data_ptr()
    b.obs_others = xo.data_ptr() if xo is not None else None
    b.self_stride[:] = [xs.stride(0), xs.stride(1), xs.stride(2)]
    b.others_stride[:] = [xo.stride(0), xo.stride(1), xo.stride(2), xo.stride(3)] if xo is not None else [0, 0, 0, 0]
    b.cyl_stride[:] = [xc.stride(0), xc.stride(1), xc.stride(2), xc.stride(3)]
    b.num_envs, b.num_steps, b.batch = N, T, B
    b.index = index.data_ptr() if index is not None else None
    b.b_values, b.b_returns = bv.data_ptr(), ret.data_ptr()
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if scal is None:
        scal = torch.empty(3, dtype=torch.float32, device=dev)
    values = torch.empty(B, A, 1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = lib.hns_critic_train_grad(C.byref(net), C.byref(b), D, A, K, float(clip_param), LOSSES[loss], float(huber_delta), C.byref(grd),
                                       scal[0:].data_ptr(), scal[1:].data_ptr(), scal[2:].data_ptr(), values.data_ptr(), ws.data_ptr(), nbytes, st)
    _check(rc, "hns_critic_train_grad")
    return CriticLoss(scal[0], scal[1], scal[2], values)


class ClippedAdam(TPAdam):
    """clip_grad_norm_(params, max_grad_norm) followed by torch.optim.Adam's step, as update_critic runs them: one launch of
    hns_adam_clipped per step for all tensors on the device (device-resident step counter, capturable), the reference's torch statements on
    the CPU.  `step(grad_norm=...)` takes the total gradient norm value_loss_and_grad returned (a 0-dim device tensor; required on the device
    unless max_grad_norm is inf or None).  state_dict() / load_state_dict() use Adam's format.  `last_grad_norm`: the unclipped norm of the
    last step (what clip_grad_norm_ returns)."""

    def __init__(self, params, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=10.0, weight_decay=0.0):
        if weight_decay != 0:
            raise NotImplementedError("ClippedAdam implements Adam with weight_decay 0")
        super().__init__(params, lr=lr, betas=betas, eps=eps)
        self.max_grad_norm = float("inf") if max_grad_norm is None else float(max_grad_norm)
        if not self.max_grad_norm >= 0:
            raise ValueError("max_grad_norm must be >= 0")
        self.last_grad_norm = None

    @torch.no_grad()
    def step(self, closure=None, grad_norm=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            self._check_group(group)
            ps = [p for p in group["params"] if p.grad is not None]
            cpu = [p for p in ps if not p.is_cuda]
            dev = [p for p in ps if p.is_cuda]
            if cpu:
                self.last_grad_norm = nn.utils.clip_grad_norm_(cpu, self.max_grad_norm)
                for p in cpu:
                    self._cpu_step(p, self._state(p, None), group)
            if dev:
                self._device_step(dev, group, grad_norm)
        return loss

    def _device_step(self, ps, group, grad_norm=None):
        devs = {p.device for p in ps}
        if len(devs) != 1:
            raise ValueError(f"ClippedAdam: the parameters of a group live on one device, not {devs}")
        dev = ps[0].device
        clip = math.isfinite(self.max_grad_norm)
        if clip:
            if grad_norm is None:
                raise ValueError("ClippedAdam.step on the device needs grad_norm= (value_loss_and_grad's) unless max_grad_norm is inf")
            if not torch.is_tensor(grad_norm) or grad_norm.device != dev or grad_norm.dtype != torch.float32 or grad_norm.numel() != 1:
                raise ValueError("grad_norm must be a one-element float32 tensor on the parameters' device")
        shared = next((self.state[p]["step"] for p in ps if len(self.state[p]) and self.state[p]["step"].device == dev), None)
        if shared is None:
            shared = torch.zeros((), dtype=torch.float32, device=dev)
        arr = (abi.HnsAdamTensor * len(ps))()
        for j, p in enumerate(ps):
            st = self._state(p, shared)
            if st["step"] is not shared:
                raise RuntimeError("ClippedAdam: the parameters of a group on one device step together (one step counter)")
            if p.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous() or p.grad.dtype != torch.float32:
                raise ValueError("ClippedAdam on the device takes contiguous float32 parameters and gradients")
            arr[j] = abi.HnsAdamTensor(p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
        beta1, beta2 = group["betas"]
        with torch.cuda.device(dev):
            rc = abi.load_library().hns_adam_clipped(arr, len(ps), shared.data_ptr(), grad_norm.data_ptr() if clip else None,
                                                     self.max_grad_norm, float(group["lr"]), float(beta1), float(beta2), float(group["eps"]),
                                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        _check(rc, "hns_adam_clipped")
        self.last_grad_norm = grad_norm
        for p in ps:
            torch.autograd.graph.increment_version(p)


def make_optimizer(critic, cfg=None):
    """The reference's critic_opt (mappo.py:198-200) as a ClippedAdam: cfg is the algo cfg (critic.lr, critic.weight_decay, max_grad_norm)."""
    get, sget = _getter(cfg), _getter(_getter(cfg)("critic", None))
    if sget("lr_scheduler", None):
        raise P.PolicyConfigError("critic.lr_scheduler is not supported")
    return ClippedAdam(critic_parameters(critic).values(), lr=float(sget("lr", 5e-4)), max_grad_norm=get("max_grad_norm", 10.0),
                       weight_decay=float(sget("weight_decay", 0.0) or 0.0))


def update_critic(critic, obs_self, obs_others, obs_cylinders, b_values, b_returns, optimizer, index=None, cfg=None, check_index=False,
                  workspace=None, out=None):
    """MAPPOPolicy.update_critic on one minibatch: loss, backward, clip_grad_norm_, Adam.  cfg: the algo cfg (clip_param, critic.use_huber_loss,
    critic.huber_delta; the reference's defaults when None).  Returns {"value_loss", "critic_grad_norm", "explained_var"} as 0-dim tensors on the
    parameters' device — the caller decides when to .item().  `optimizer`: a ClippedAdam (make_optimizer).  The index is NOT range-checked
    by default (make_dataset_naive's permutations are in range by construction; the check is a host synchronisation per minibatch, and the
    kernel skips an env-step outside the rollout): pass check_index=True for an index of another origin.  `workspace`, `out`:
    value_loss_and_grad's."""
    if not isinstance(optimizer, ClippedAdam):
        raise TypeError(f"update_critic takes a ClippedAdam (critic_train.make_optimizer), not {type(optimizer).__name__}: the clip and the "
                        "step are one launch that needs the gradient norm")
    P.check_config(cfg)
    get, sget = _getter(cfg), _getter(_getter(cfg)("critic", None))
    if float(sget("weight_decay", 0.0) or 0.0) != 0:
        raise NotImplementedError("critic.weight_decay != 0 is not supported")
    if int(sget("num_critics", 1) or 1) != 1:
        raise P.PolicyConfigError("critic.num_critics > 1 is not supported")
    for group in optimizer.param_groups:
        if group.get("weight_decay", 0) != 0:
            raise NotImplementedError("weight_decay != 0 is not supported")
    res = value_loss_and_grad(critic, obs_self, obs_others, obs_cylinders, b_values, b_returns, index, clip_param=float(get("clip_param", 0.1)),
                              loss="huber" if sget("use_huber_loss", True) else "mse", huber_delta=float(sget("huber_delta", 10.0)),
                              check_index=check_index, workspace=workspace, out=out)
    optimizer.step(grad_norm=res.grad_norm)
    norm = optimizer.last_grad_norm if getattr(optimizer, "last_grad_norm", None) is not None else res.grad_norm
    return {"value_loss": res.value_loss, "critic_grad_norm": norm, "explained_var": res.explained_var}
