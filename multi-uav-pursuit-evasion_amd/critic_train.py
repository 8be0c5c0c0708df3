"""The MAPPO critic's update on the device: MAPPOPolicy.update_critic (learning/mappo.py:326-352) for make_critic's network at
cfg/algo/mappo.yaml's defaults (critic_input: obs, no rnn, weight_decay 0).

`value_loss_and_grad(critic, obs_self, obs_others, obs_cylinders, b_values, b_returns, index)` is update_critic up to `backward()`: device
tensors go to ONE call of `hns_critic_train_grad` (forward + loss partials, the branch decision of the max of the two mean losses, the
encoder's backward pass, the weight-gradient products, fixed-order sums) that fills every parameter's `.grad` in its PyTorch layout and
returns value_loss, explained_var and the total gradient norm as 0-dim device tensors — no autograd graph, no host synchronisation.  `index`
reads a minibatch of `make_dataset_naive` (mappo.py:493-513, seq_len 1) in place from the rollout's [N, T, A, ...] observations.

`ClippedAdam` (optim's, re-exported here) is clip_grad_norm_ + torch.optim.Adam in one call of `hns_adam_clipped`.  What this update
shares with the actor's — the batch checks, the preparation of the C call, the encoder's restatement — lives in `policy_train`.

The data-parallel form splits the call where the branch of the max is decided: `value_loss_sums` is the forward pass and the
five fp64 sums of this rank's rows (`hns_critic_train_sums`); the caller adds the ranks' sums; `value_loss_and_grad(sums=, global_rows=)`
decides on the union's sums and scales the rows by 1 / global_rows (`hns_critic_train_grad_global`), so the ranks' gradients add up to the
union's in a `policy_train.GradBucket`.  `update_critic(group=)` runs the whole sequence.

`value_loss_and_grad_central` / `update_critic_central` are the same two functions for the centralised critic (critic_input: state): ONE call
of `hns_critic_train_grad_central` on tiles of env-steps, the state read in place.

`update_critic` is the reference's function.  CPU tensors run the reference's torch statements throughout (CPU tests, gloo runs — not the
hot path).  DESIGN.md §7.4."""
import collections
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import abi
from . import policy as P
from . import policy_train as PT
from .policy_train import ClippedAdam

CriticLoss = collections.namedtuple("CriticLoss", ["value_loss", "explained_var", "grad_norm", "values"])
CriticSums = collections.namedtuple("CriticSums", ["sums", "values"])
LOSSES = {"huber": abi.HNS_CRITIC_LOSS_HUBER, "mse": abi.HNS_CRITIC_LOSS_MSE}


def critic_parameters(critic):
    """The critic's tensors by hns_policy_net field, in the order the module registers them (clip_grad_norm_'s order)."""
    return P.parse_parameters(critic, P.CRITIC_NAMES, "critic")


def _gather(xs, xo, xc, b_values, b_returns, index):
    N, T, A, D = xs.shape
    xs, xc = xs.reshape(N * T, A, 1, D), xc.reshape(N * T, A, xc.shape[3], 5)
    xo = xo.reshape(N * T, A, A - 1, 3) if xo is not None else None
    bv, ret = b_values.reshape(N * T, A, 1), b_returns.reshape(N * T, A, 1)
    if index is not None:
        xs, xc, bv, ret = xs[index], xc[index], bv[index], ret[index]
        xo = xo[index] if xo is not None else None
    return xs, xo, xc, bv, ret


def _sum_loss64(x, loss, huber_delta):
    """sum loss(x) in fp64 from fp32 differences' operands, as hns_critic_kernel<false> forms its partials."""
    ax = x.abs()
    return (x * x).sum() if loss == "mse" else torch.where(ax < huber_delta, 0.5 * x * x, huber_delta * (ax - 0.5 * huber_delta)).sum()


def _torch_sums(p, xs, xo, xc, b_values, b_returns, index, clip_param, loss, huber_delta):
    """value_loss_sums on the CPU: the five sums of hns_critic_train_sums, fp64 from the fp32 values."""
    xs, xo, xc, bv, ret = _gather(xs, xo, xc, b_values, b_returns, index)
    with torch.no_grad():
        values = F.linear(PT.encoder(p, xs, xo, xc), p["head_w"], p["head_b"])
        clipped = bv + (values - bv).clamp(-clip_param, clip_param)
        v, c, r = values.double(), clipped.double(), ret.double()
        sums = torch.stack([_sum_loss64(v - r, loss, huber_delta), _sum_loss64(c - r, loss, huber_delta), ((v - r) ** 2).sum(), r.sum(), (r * r).sum()])
    return CriticSums(sums, values)


def _torch_loss_and_grad_global(p, xs, xo, xc, b_values, b_returns, index, clip_param, loss, huber_delta, sums, global_rows, group, bucket):
    """hns_critic_train_grad_global on the CPU: the branch, value_loss and explained_var from the union's `sums`, the gradient of this rank's
    rows of the chosen branch's sum over global_rows."""
    xs, xo, xc, bv, ret = _gather(xs, xo, xc, b_values, b_returns, index)
    n = float(global_rows)
    S = sums.double().tolist()
    lo, lc = S[0] / n, S[1] / n
    w0, w1 = (1.0, 0.0) if lo > lc else ((0.0, 1.0) if lo < lc else (0.5, 0.5))
    leaves = {k: v.detach().requires_grad_(True) for k, v in p.items()}
    values = F.linear(PT.encoder(leaves, xs, xo, xc), leaves["head_w"], leaves["head_b"])
    # the loss and its per-row derivative in fp64 from the fp32 values, as the kernel forms its loss partials: v - ret is not rounded to fp32
    # before the 1 / n, so a rank's part carries the rounding of its fp32 backward pass alone
    v64, bv64, ret64 = values.double(), bv.double(), ret.double()
    clipped = bv64 + (v64 - bv64).clamp(-clip_param, clip_param)
    loss_fn = nn.HuberLoss(delta=huber_delta, reduction="sum") if loss == "huber" else nn.MSELoss(reduction="sum")
    total = (w0 * loss_fn(ret64, v64) + w1 * loss_fn(ret64, clipped)) / n
    grads = torch.autograd.grad(total, list(leaves.values()))
    for t, g in zip(p.values(), grads):
        t.grad = g
    if bucket is not None:
        bucket.adopt()
    grad_norm = PT.finish_global(bucket, group)
    value_loss = torch.tensor(max(lo, lc), dtype=torch.float32)
    explained_var = torch.tensor(1.0 - (S[2] / n) / ((S[4] - S[3] * S[3] / n) / (n - 1.0)), dtype=torch.float32)
    return CriticLoss(value_loss, explained_var, grad_norm, values.detach())


def _torch_loss_and_grad(p, xs, xo, xc, b_values, b_returns, index, clip_param, loss, huber_delta):
    """update_critic's statements (mappo.py:328-341) on the gathered minibatch; autograd through policy_train's encoder."""
    xs, xo, xc, bv, ret = _gather(xs, xo, xc, b_values, b_returns, index)
    leaves = {k: v.detach().requires_grad_(True) for k, v in p.items()}
    values = F.linear(PT.encoder(leaves, xs, xo, xc), leaves["head_w"], leaves["head_b"])
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


def value_loss_sums(critic, obs_self, obs_others, obs_cylinders, b_values, b_returns, index=None, clip_param=0.1, loss="huber", huber_delta=10.0,
                    check_index=True, workspace=None):
    """The forward half of a data-parallel value_loss_and_grad: CriticSums(sums, values) with sums the five fp64 device values of
    hns_critic_train_sums over THIS rank's rows (sum loss(v - ret), sum loss(clipped - ret), sum (v - ret)^2, sum ret, sum ret^2) and values
    [B, A, 1].  No gradient is touched.  The caller adds the ranks' sums (one SUM all-reduce) and passes the result to
    value_loss_and_grad(sums=, global_rows=).  Arguments and refusals: value_loss_and_grad's."""
    if loss not in LOSSES:
        raise ValueError(f"loss must be 'huber' or 'mse', not {loss!r}")
    if not clip_param >= 0 or (loss == "huber" and not huber_delta > 0):
        raise ValueError("clip_param must be >= 0 and huber_delta > 0")
    p = critic_parameters(critic)
    xs, xo, xc = PT.as_rollout(obs_self, obs_others, obs_cylinders)
    shape = PT.validate("critic", p, xs, xo, xc, (("b_values", b_values, 1), ("b_returns", b_returns, 1)), index, check_index)
    if not xs.is_cuda:
        return _torch_sums(p, xs, xo, xc, b_values, b_returns, index, float(clip_param), loss, float(huber_delta))
    lib = abi.load_library()
    bv, ret = b_values.contiguous(), b_returns.contiguous()
    _, _, A, D, K = shape
    dev = xs.device
    B = index.numel() if index is not None else shape[0] * shape[1]
    for f, t in p.items():
        if t.data_ptr() % 16:
            raise ValueError(f"critic parameter {f} must be 16-byte aligned")
    nbytes = lib.hns_critic_train_workspace_bytes(B * A, D, A, K)
    if nbytes == 0:
        raise ValueError(f"shape outside the kernel's limits: {B * A} rows, self_dim {D}, {A} agents, {K} cylinders")
    ws = PT.check_workspace(workspace, nbytes, dev) if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    net = abi.HnsPolicyNet()
    for f, t in p.items():
        setattr(net, f, t.data_ptr())
    b = PT.fill_batch(abi.HnsCriticBatch, xs, xo, xc, index, shape)
    b.b_values, b.b_returns = bv.data_ptr(), ret.data_ptr()
    sums = torch.empty(5, dtype=torch.float64, device=dev)
    values = torch.empty(B, A, 1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.hns_critic_train_sums(C.byref(net), C.byref(b), D, A, K, float(clip_param), LOSSES[loss], float(huber_delta), sums.data_ptr(),
                                       values.data_ptr(), ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    abi.check(rc, "hns_critic_train_sums")
    return CriticSums(sums, values)


def value_loss_and_grad(critic, obs_self, obs_others, obs_cylinders, b_values, b_returns, index=None, clip_param=0.1, loss="huber",
                        huber_delta=10.0, check_index=True, workspace=None, out=None, sums=None, global_rows=None, group=None, bucket=None):
    """The clipped value loss of the critic on a minibatch and every parameter's .grad (as zero_grad() + backward() leave them, before
    clip_grad_norm_).  Returns CriticLoss(value_loss, explained_var, grad_norm: 0-dim tensors; values [B, A, 1]).

    obs_*: the rollout's [N, T, A, ...] observations (state_self [N, T, A, D] or [N, T, A, 1, D]; state_others None with one agent) or a
    flat [R, A, ...] batch, read in place; b_values, b_returns: [N, T, A, 1] (any shape of N T A values); index: int64 [B] env-steps of the
    flattened [N T] (None: all).  `check_index` range-checks the index (one host synchronisation; skipped inside a graph capture).
    `workspace`: a uint8 device tensor of at least hns_critic_train_workspace_bytes bytes, 256-byte aligned, instead of one allocated per call;
    `out`: three fp32 device values that receive value_loss, explained_var and grad_norm (the returned scalars are views of it) instead of a
    tensor of the call's own.  Both are ignored on the CPU.

    `sums`, `global_rows` (both None: the call above, untouched): this minibatch is one rank's part of a union of `global_rows` agent rows
    whose five fp64 sums are `sums` (value_loss_sums' over all ranks, added): hns_critic_train_grad_global takes the branch, value_loss and
    explained_var from them — the same on every rank — and the gradients are this rank's part, which adds up over the ranks to the union's.
    `values` is None on the device (value_loss_sums returned them).  `bucket`: the critic's `policy_train.GradBucket`; grad_norm is then the
    bucket's norm (None without one).  `group`: the bucket is all-reduced (SUM) over it first."""
    if loss not in LOSSES:
        raise ValueError(f"loss must be 'huber' or 'mse', not {loss!r}")
    if not clip_param >= 0 or (loss == "huber" and not huber_delta > 0):
        raise ValueError("clip_param must be >= 0 and huber_delta > 0")
    if (sums is None) != (global_rows is None):
        raise ValueError("sums= and global_rows= travel together: the union's five sums and its row count")
    p = critic_parameters(critic)
    xs, xo, xc = PT.as_rollout(obs_self, obs_others, obs_cylinders)
    shape = PT.validate("critic", p, xs, xo, xc, (("b_values", b_values, 1), ("b_returns", b_returns, 1)), index, check_index)
    PT.check_global("critic", p, global_rows, (index.numel() if index is not None else shape[0] * shape[1]) * shape[2], group, bucket)
    if sums is not None and (not torch.is_tensor(sums) or sums.dtype != torch.float64 or sums.numel() != 5 or sums.device != xs.device or
                             not sums.is_contiguous()):
        raise ValueError(f"sums must be five contiguous float64 values on {xs.device}")
    if not xs.is_cuda:
        if sums is not None:
            return _torch_loss_and_grad_global(p, xs, xo, xc, b_values, b_returns, index, float(clip_param), loss, float(huber_delta), sums,
                                               global_rows, group, bucket)
        return _torch_loss_and_grad(p, xs, xo, xc, b_values, b_returns, index, float(clip_param), loss, float(huber_delta))
    lib = abi.load_library()
    bv, ret = b_values.contiguous(), b_returns.contiguous()
    net, grd, b, ws, nbytes, scal, B, st = PT.prepare_call("critic", p, xs, xo, xc, index, shape, lib.hns_critic_train_workspace_bytes, workspace,
                                                           out, 3, abi.HnsCriticBatch)
    _, _, A, D, K = shape
    b.b_values, b.b_returns = bv.data_ptr(), ret.data_ptr()
    if sums is not None:
        with torch.cuda.device(xs.device):
            rc = lib.hns_critic_train_grad_global(C.byref(net), C.byref(b), D, A, K, float(clip_param), LOSSES[loss], float(huber_delta), C.byref(grd),
                                                  scal[0:].data_ptr(), scal[1:].data_ptr(), None, None, ws.data_ptr(), nbytes, st, sums.data_ptr(),
                                                  int(global_rows))
        abi.check(rc, "hns_critic_train_grad_global")
        norm = PT.finish_global(bucket, group, scal[2:3])
        return CriticLoss(scal[0], scal[1], scal[2] if norm is not None else None, None)
    values = torch.empty(B, A, 1, dtype=torch.float32, device=xs.device)
    with torch.cuda.device(xs.device):
        rc = lib.hns_critic_train_grad(C.byref(net), C.byref(b), D, A, K, float(clip_param), LOSSES[loss], float(huber_delta), C.byref(grd),
                                       scal[0:].data_ptr(), scal[1:].data_ptr(), scal[2:].data_ptr(), values.data_ptr(), ws.data_ptr(), nbytes, st)
    abi.check(rc, "hns_critic_train_grad")
    return CriticLoss(scal[0], scal[1], scal[2], values)


def critic_cfg(cfg, central=False):
    """The refusals of the critic's part of the algo cfg (policy.check_config's — central: policy.check_config_central's —, then
    critic.lr_scheduler, critic.weight_decay, critic.num_critics); returns the cfg's and the critic section's getters."""
    (P.check_config_central if central else P.check_config)(cfg)
    sget = PT.getter(PT.getter(cfg)("critic", None))
    if sget("lr_scheduler", None):
        raise P.PolicyConfigError("critic.lr_scheduler is not supported")
    if float(sget("weight_decay", 0.0) or 0.0) != 0:
        raise NotImplementedError("critic.weight_decay != 0 is not supported")
    if int(sget("num_critics", 1) or 1) != 1:
        raise P.PolicyConfigError("critic.num_critics > 1 is not supported")
    return PT.getter(cfg), sget


def make_optimizer(critic, cfg=None):
    """The reference's critic_opt (mappo.py:198-200) as a ClippedAdam: cfg is the algo cfg (critic.lr, critic.weight_decay, max_grad_norm).
    The centralised critic (its parameters embed state_drones) is taken with its own 20 tensors and critic_input: state."""
    central = is_central(critic)
    get, sget = critic_cfg(cfg, central=central)
    return ClippedAdam((central_critic_parameters(critic) if central else critic_parameters(critic)).values(), lr=float(sget("lr", 5e-4)), max_grad_norm=get("max_grad_norm", 10.0),
                       weight_decay=float(sget("weight_decay", 0.0) or 0.0))


def update_critic(critic, obs_self, obs_others, obs_cylinders, b_values, b_returns, optimizer, index=None, cfg=None, check_index=False,
                  workspace=None, out=None, sums=None, global_rows=None, group=None, bucket=None):
    """MAPPOPolicy.update_critic on one minibatch: loss, backward, clip_grad_norm_, Adam.  cfg: the algo cfg (clip_param, critic.use_huber_loss,
    critic.huber_delta; the reference's defaults when None).  Returns {"value_loss", "critic_grad_norm", "explained_var"} as 0-dim tensors on the
    parameters' device — the caller decides when to .item().  `optimizer`: a ClippedAdam (make_optimizer).  The index is NOT range-checked
    by default (make_dataset_naive's permutations are in range by construction; the check is a host synchronisation per minibatch, and the
    kernel skips an env-step outside the rollout): pass check_index=True for an index of another origin.  `workspace`, `out`:
    value_loss_and_grad's.  `global_rows`, `bucket`: one rank's part of a data-parallel update over a union of `global_rows` rows.  With
    `group` the call runs value_loss_sums, the SUM all-reduce of the five values, value_loss_and_grad(sums=, group=) and the step; `sums`
    given instead: the caller added the ranks' sums itself."""
    if global_rows is not None and bucket is None:
        raise ValueError("update_critic with global_rows= steps on the bucket's norm: pass bucket=")
    if global_rows is not None and sums is None and group is None:
        raise ValueError("update_critic with global_rows= needs the union's sums= or the group= to add them over")
    get, sget = PT.check_optimizer(optimizer, "update_critic", "critic_train.make_optimizer", critic_cfg, cfg)
    kw = dict(clip_param=float(get("clip_param", 0.1)), loss="huber" if sget("use_huber_loss", True) else "mse",
              huber_delta=float(sget("huber_delta", 10.0)), check_index=check_index, workspace=workspace)
    if global_rows is not None and sums is None:
        from . import sharding
        sums = sharding.all_reduce_sum(value_loss_sums(critic, obs_self, obs_others, obs_cylinders, b_values, b_returns, index, **kw).sums, group)
    res = value_loss_and_grad(critic, obs_self, obs_others, obs_cylinders, b_values, b_returns, index, out=out, sums=sums, global_rows=global_rows,
                              group=group, bucket=bucket, **kw)
    return {"value_loss": res.value_loss, "critic_grad_norm": PT.clipped_step(optimizer, res.grad_norm), "explained_var": res.explained_var}


# ---------------------------------------------------------------------------------------------------------------------------------------
# The centralised critic (critic_input: state; policy.CentralCriticDevicePolicy): ONE row per env-step over the state —
# the A rows of state_drones through one embedding, then the K cylinders — and v_out = Linear(128, A).  b_values, b_returns, the value
# loss (the mean over batch x A values), ValueNorm and GAE are the obs critic's.

def central_critic_parameters(critic):
    """The centralised critic's 20 tensors by hns_policy_net field (embed_self_*: the state_drones embedding), in registration order."""
    return P.parse_parameters_central(critic, "critic")[0]


def is_central(critic):
    """Whether `critic` (any source `parse_parameters` reads) is the centralised critic: it embeds state_drones."""
    return any(".state_drones." in "." + P._strip(k) for k in P._flatten(critic))


def _central_state(state_drones, state_cylinders):
    """(state_drones [N, T, A, D], the state's cylinders [N, T, K, 5]) as views: a flat [R, ...] batch is [R, 1, ...]; cylinders given as the
    rollout's obs_cylinders [N, T, A, K, 5] are agent 0's rows of it, in place."""
    sd, sc = state_drones, state_cylinders
    if sd.dim() == 3:
        sd, sc = sd.unsqueeze(1), sc.unsqueeze(1)
    if sd.dim() != 4:
        raise ValueError(f"state_drones must be [N, T, A, D] or [R, A, D], not {tuple(state_drones.shape)}")
    if sc.dim() == 5:
        sc = sc[:, :, 0]
    return sd, sc


def _validate_central(p, sd, sc, b_values, b_returns, index, check_index):
    """policy_train.validate's refusals for the centralised critic's tensors; returns (N, T, A, D, K)."""
    for k, t in p.items():
        if not t.is_contiguous():
            raise ValueError(f"critic parameter {k} must be contiguous")
    D, A = int(p["embed_self_w"].shape[1]), int(p["head_w"].shape[0])
    N, T, Ax, Dx = sd.shape
    if Dx != D:
        raise ValueError(f"state_drones rows have {Dx} values, the critic takes {D}")
    if Ax != A:
        raise ValueError(f"state_drones holds {Ax} drones, v_out has {A} rows")
    if sc.dim() != 4 or tuple(sc.shape[:2]) != (N, T) or sc.shape[-1] != 5 or not 1 <= sc.shape[2] <= abi.HNS_MAX_CYLINDERS:
        raise ValueError(f"the state's cylinders must be [{N}, {T}, K, 5] (or the rollout's [{N}, {T}, {A}, K, 5]) with K in "
                         f"[1, {abi.HNS_MAX_CYLINDERS}], not {tuple(sc.shape)}")
    for name, t in (("state_drones", sd), ("cylinders", sc), ("b_values", b_values), ("b_returns", b_returns)):
        if t.dtype != torch.float32:
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
        if check_index and not (sd.is_cuda and torch.cuda.is_current_stream_capturing()):
            lo, hi = torch.stack([index.min(), index.max()]).tolist()     # one host synchronisation
            if lo < 0 or hi >= steps:
                raise IndexError(f"index values [{lo}, {hi}] outside the {steps} env-steps of the rollout")
    devs = {t.device for t in (*p.values(), sd, sc, b_values, b_returns)} | ({index.device} if index is not None else set())
    if len(devs) != 1:
        raise ValueError(f"parameters, state, b_values, b_returns and index must share one device, not {devs}")
    return N, T, A, D, int(sc.shape[2])


def _torch_loss_and_grad_central(p, sd, sc, b_values, b_returns, index, clip_param, loss, huber_delta):
    """update_critic's statements (mappo.py:328-341) on the gathered minibatch of the centralised critic: values [B, A, 1] from ONE encoder
    row per env-step (Critic.forward with centralized=True, mappo.py:644-660); autograd through policy_train's encoder.  An index entry
    outside [0, N T) — reachable with check_index=False only — contributes nothing, as include/hns.h documents for hns_critic_batch.index and
    as the kernel does (torch's own gather would read a negative entry from the end and raise on one past the end): its A values join no
    sum, the means still divide by the whole minibatch's batch x A.  Its rows of `values` are zero HERE; on the device they are whatever the
    freshly allocated tensor held (the kernel writes live rows only)."""
    N, T, A, D = sd.shape
    sd, sc = sd.reshape(N * T, A, D), sc.reshape(N * T, sc.shape[2], 5)
    bv, ret = b_values.reshape(N * T, A, 1), b_returns.reshape(N * T, A, 1)
    live = None
    if index is not None:
        live = (index >= 0) & (index < N * T)
        if bool(live.all()):
            live = None
        else:
            index = index[live]
        sd, sc, bv, ret = sd[index], sc[index], bv[index], ret[index]
    leaves = {k: v.detach().requires_grad_(True) for k, v in p.items()}
    values = F.linear(PT.encoder(leaves, sd, None, sc), leaves["head_w"], leaves["head_b"]).unsqueeze(-1)
    clipped = bv + (values - bv).clamp(-clip_param, clip_param)
    if live is not None:
        # sums over the live values divided by the whole minibatch's count, as the kernel's partials; the all-live statements below stay as
        # they are for their bits (mean reductions round otherwise than sum / n)
        n = float(live.numel() * A)
        loss_fn = nn.HuberLoss(delta=huber_delta, reduction="sum") if loss == "huber" else nn.MSELoss(reduction="sum")
        value_loss = torch.max(loss_fn(ret, values) / n, loss_fn(ret, clipped) / n)
        grads = torch.autograd.grad(value_loss, list(leaves.values()))
        for t, g in zip(p.values(), grads):
            t.grad = g
        with torch.no_grad():
            grad_norm = nn.utils.clip_grad_norm_(list(p.values()), float("inf"))
            v64, r64 = values.double(), ret.double()
            explained_var = (1 - (((v64 - r64) ** 2).sum() / n) / (((r64 * r64).sum() - r64.sum() ** 2 / n) / (n - 1.0))).to(torch.float32)
            out = values.new_zeros(live.numel(), A, 1)
            out[live] = values.detach()
        return CriticLoss(value_loss.detach(), explained_var, grad_norm, out)
    loss_fn = nn.HuberLoss(delta=huber_delta) if loss == "huber" else nn.MSELoss()
    l_clip = loss_fn(ret, clipped)
    l_orig = loss_fn(ret, values)
    value_loss = torch.max(l_orig, l_clip)
    grads = torch.autograd.grad(value_loss, list(leaves.values()))
    for t, g in zip(p.values(), grads):
        t.grad = g
    with torch.no_grad():
        grad_norm = nn.utils.clip_grad_norm_(list(p.values()), float("inf"))
        # in fp64 from the fp32 values, as the kernel's loss partials: 1 - mse / var cancels, and in fp32 the rounding of that difference
        # (one ulp of 1) is many ulps of a small explained variance
        explained_var = (1 - F.mse_loss(values.double(), ret.double()) / ret.double().var()).to(torch.float32)
    return CriticLoss(value_loss.detach(), explained_var, grad_norm, values.detach())


def value_loss_and_grad_central(critic, state_drones, state_cylinders, b_values, b_returns, index=None, clip_param=0.1, loss="huber",
                                huber_delta=10.0, check_index=True, workspace=None, out=None):
    """`value_loss_and_grad` for the centralised critic, ONE call of `hns_critic_train_grad_central`: the clipped value loss over the
    minibatch's batch x A values and every parameter's .grad.  Returns CriticLoss(value_loss, explained_var, grad_norm; values [B, A, 1]).

    state_drones: the rollout's [N, T, A, D] (or a flat [R, A, D]), read in place; state_cylinders: [N, T, K, 5] — any strided view, so the
    stored obs_cylinders[:, :, 0] costs no copy — or the rollout's obs_cylinders [N, T, A, K, 5] itself, of which agent 0's rows are read;
    b_values, b_returns, index, check_index, workspace (hns_critic_train_central_workspace_bytes bytes) and out: value_loss_and_grad's.
    With check_index=False an index entry outside the rollout contributes nothing to value_loss, explained_var, grad_norm and the gradients,
    on the device and on the CPU alike (include/hns.h); its rows of `values` are unspecified (the device leaves them unwritten, the CPU
    path zeroes them)."""
    if loss not in LOSSES:
        raise ValueError(f"loss must be 'huber' or 'mse', not {loss!r}")
    if not clip_param >= 0 or (loss == "huber" and not huber_delta > 0):
        raise ValueError("clip_param must be >= 0 and huber_delta > 0")
    p = central_critic_parameters(critic)
    sd, sc = _central_state(state_drones, state_cylinders)
    shape = _validate_central(p, sd, sc, b_values, b_returns, index, check_index)
    if not sd.is_cuda:
        return _torch_loss_and_grad_central(p, sd, sc, b_values, b_returns, index, float(clip_param), loss, float(huber_delta))
    lib = abi.load_library()
    bv, ret = b_values.contiguous(), b_returns.contiguous()
    _, _, A, D, K = shape
    # the batch struct reinterpreted (include/hns.h): obs_self is state_drones, obs_cylinders the [N, T, K, 5] view with a unit agent axis
    net, grd, b, ws, nbytes, scal, B, st = PT.prepare_call(
        "critic", p, sd, None, sc.unsqueeze(2), index, shape,
        lambda rows, D_, A_, K_: lib.hns_critic_train_central_workspace_bytes(rows // A_, D_, A_, K_), workspace, out, 3, abi.HnsCriticBatch)
    b.b_values, b.b_returns = bv.data_ptr(), ret.data_ptr()
    values = torch.empty(B, A, 1, dtype=torch.float32, device=sd.device)
    with torch.cuda.device(sd.device):
        rc = lib.hns_critic_train_grad_central(C.byref(net), C.byref(b), D, A, K, float(clip_param), LOSSES[loss], float(huber_delta), C.byref(grd),
                                               scal[0:].data_ptr(), scal[1:].data_ptr(), scal[2:].data_ptr(), values.data_ptr(), ws.data_ptr(), nbytes,
                                               st)
    abi.check(rc, "hns_critic_train_grad_central")
    return CriticLoss(scal[0], scal[1], scal[2], values)


def update_critic_central(critic, state_drones, state_cylinders, b_values, b_returns, optimizer, index=None, cfg=None, check_index=False,
                          workspace=None, out=None):
    """MAPPOPolicy.update_critic on one minibatch with the centralised critic: loss, backward, clip_grad_norm_, Adam.  `update_critic`'s
    cfg, info dict ({"value_loss", "critic_grad_norm", "explained_var"} as 0-dim tensors), optimizer, index and workspace handling; the
    state arguments are value_loss_and_grad_central's.  A process group is not supported (there is no data-parallel form)."""
    get, sget = PT.check_optimizer(optimizer, "update_critic_central", "critic_train.make_optimizer", lambda c: critic_cfg(c, central=True), cfg)
    res = value_loss_and_grad_central(critic, state_drones, state_cylinders, b_values, b_returns, index, clip_param=float(get("clip_param", 0.1)),
                                      loss="huber" if sget("use_huber_loss", True) else "mse", huber_delta=float(sget("huber_delta", 10.0)),
                                      check_index=check_index, workspace=workspace, out=out)
    return {"value_loss": res.value_loss, "critic_grad_norm": PT.clipped_step(optimizer, res.grad_norm), "explained_var": res.explained_var}
