"""The MAPPO actor's update on the device: MAPPOPolicy.update_actor (learning/mappo.py:271-324) for make_ppo_actor's network at
cfg/algo/mappo.yaml's defaults (share_actor, no tanh, no rnn, a 4-dim continuous action, DiagGaussian: fc_mean 128 -> 4 and a free log_std).

`policy_loss_and_grad(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, index)` is update_actor up to
`backward()`: device tensors go to ONE call of `hns_actor_train_grad` (one pass over the tiles: forward, log-probability, ratio, clipped
surrogate with its per-row backward weight, the encoder's backward pass; then the weight-gradient products and fixed-order sums) that fills
every parameter's `.grad` in its PyTorch layout and returns policy_loss, entropy, ESS and the total gradient norm as 0-dim device tensors —
no autograd graph, no host synchronisation.  `index` reads a minibatch of `make_dataset_naive` in place from the rollout's [N, T, A, ...]
tensors, as critic_train does.

The step is critic_train's `ClippedAdam` (clip_grad_norm_ + torch.optim.Adam in one launch) over the actor's 23 tensors; it bumps the
parameters' version counters, so `policy.DevicePolicy` re-packs its operand image before the next forward pass.

`update_actor` is the reference's function.  CPU tensors run the reference's torch statements throughout (CPU tests, gloo runs — not the
hot path).  DESIGN.md §7.5."""
import collections
import ctypes as C

import torch
import torch.distributions as D
import torch.nn as nn
import torch.nn.functional as F

from . import abi
from . import policy as P
from .critic_train import ClippedAdam, _as_rollout, _check, _check_out, _check_workspace, _encoder, _getter

ActorLoss = collections.namedtuple("ActorLoss", ["policy_loss", "entropy", "ess", "grad_norm", "log_probs"])


def actor_parameters(actor):
    """The actor's tensors by hns_policy_net field, in the order the parameters are registered (clip_grad_norm_'s order)."""
    return P.parse_parameters(actor, P.ACTOR_NAMES, "actor")


def _validate(p, xs, xo, xc, action, log_probs_old, advantages, index, check_index):
    """Every refusal of hns_actor_train_grad, raised here before anything is launched."""
    for k, t in p.items():
        if not t.is_contiguous():
            raise ValueError(f"actor parameter {k} must be contiguous")
    D_ = int(p["embed_self_w"].shape[1])
    N, T, A, Dx = xs.shape
    if Dx != D_:
        raise ValueError(f"state_self rows have {Dx} values, the actor takes {D_}")
    if not 1 <= A <= abi.HNS_MAX_AGENTS:
        raise ValueError(f"{A} agents outside [1, {abi.HNS_MAX_AGENTS}]")
    has_others = "embed_others_w" in p
    if (xo is not None) != has_others or (A > 1) != has_others:
        raise ValueError(f"{A} agents: state_others is {'required' if A > 1 else 'absent'} for this network")
    if xo is not None and tuple(xo.shape) != (N, T, A, A - 1, 3):
        raise ValueError(f"state_others must be [{N}, {T}, {A}, {A - 1}, 3], not {tuple(xo.shape)}")
    if xc.dim() != 5 or tuple(xc.shape[:3]) != (N, T, A) or xc.shape[-1] != 5 or not 1 <= xc.shape[3] <= abi.HNS_MAX_CYLINDERS:
        raise ValueError(f"cylinders must be [{N}, {T}, {A}, K, 5] with K in [1, {abi.HNS_MAX_CYLINDERS}], not {tuple(xc.shape)}")
    for name, t in (("state_self", xs), ("state_others", xo), ("cylinders", xc), ("action", action), ("log_probs_old", log_probs_old),
                    ("advantages", advantages)):
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, not {t.dtype}")
    steps = N * T
    if steps == 0:
        raise ValueError("the rollout holds no env-step")
    if action.numel() != steps * A * P.ACTION_DIM or action.shape[-1] != P.ACTION_DIM:
        raise ValueError(f"action must hold [N * T, A, {P.ACTION_DIM}] = [{steps}, {A}, {P.ACTION_DIM}] values, not {tuple(action.shape)}")
    for name, t in (("log_probs_old", log_probs_old), ("advantages", advantages)):
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
    devs = {t.device for t in (*p.values(), xs, xc, action, log_probs_old, advantages)} | ({xo.device} if xo is not None else set()) | \
        ({index.device} if index is not None else set())
    if len(devs) != 1:
        raise ValueError(f"parameters, observations, action, log_probs_old, advantages and index must share one device, not {devs}")
    return N, T, A, D_, int(xc.shape[3])


def _torch_loss_and_grad(p, xs, xo, xc, action, log_probs_old, advantages, index, clip_param, entropy_coef):
    """update_actor's statements (mappo.py:293-318) on the gathered minibatch, Actor.forward(eval_action=True) and DiagGaussian.forward
    (mappo.py:612-624, distributions.py:78-82) in front of them; autograd through critic_train's encoder."""
    N, T, A, D_ = xs.shape
    xs, xc = xs.reshape(N * T, A, 1, D_), xc.reshape(N * T, A, xc.shape[3], 5)
    xo = xo.reshape(N * T, A, A - 1, 3) if xo is not None else None
    action = action.reshape(N * T, A, P.ACTION_DIM)
    log_probs_old, advantages = log_probs_old.reshape(N * T, A, 1), advantages.reshape(N * T, A, 1)
    if index is not None:
        xs, xc, action, log_probs_old, advantages = xs[index], xc[index], action[index], log_probs_old[index], advantages[index]
        xo = xo[index] if xo is not None else None
    leaves = {k: v.detach().requires_grad_(True) for k, v in p.items()}
    action_mean = F.linear(_encoder(leaves, xs, xo, xc), leaves["head_w"], leaves["head_b"])
    action_std = torch.broadcast_to(torch.exp(leaves["log_std"]), action_mean.shape)
    action_dist = D.Independent(D.Normal(action_mean, action_std, validate_args=False), 1, validate_args=False)
    log_probs_new = action_dist.log_prob(action).unsqueeze(-1)
    dist_entropy = action_dist.entropy().unsqueeze(-1)
    ratio = torch.exp(log_probs_new - log_probs_old)
    surr1 = ratio * advantages
    surr2 = torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param) * advantages
    policy_loss = - torch.mean(torch.min(surr1, surr2) * P.ACTION_DIM)
    entropy_loss = - torch.mean(dist_entropy)
    grads = torch.autograd.grad(policy_loss + entropy_loss * entropy_coef, list(leaves.values()))
    for t, g in zip(p.values(), grads):
        t.grad = g
    with torch.no_grad():
        grad_norm = nn.utils.clip_grad_norm_(list(p.values()), float("inf"))      # the total norm as clip_grad_norm_ forms it; scales by 1
        ess = (2 * ratio.logsumexp(0) - (2 * ratio).logsumexp(0)).exp().mean() / ratio.shape[0]
    return ActorLoss(policy_loss.detach(), -entropy_loss.detach(), ess, grad_norm, log_probs_new.detach())


def policy_loss_and_grad(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, index=None, clip_param=0.1,
                         entropy_coef=0.001, check_index=True, workspace=None, out=None):
    """The clipped PPO surrogate of the actor on a minibatch (plus entropy_coef times the entropy loss) and every parameter's .grad (as
    zero_grad() + backward() leave them, before clip_grad_norm_).  Returns ActorLoss(policy_loss, entropy, ess, grad_norm: 0-dim tensors;
    log_probs [B, A, 1]: the new log-probabilities of the stored actions).

    obs_*: the rollout's [N, T, A, ...] observations or a flat [R, A, ...] batch, read in place (critic_train.value_loss_and_grad's
    layouts); action [N, T, A, 4], log_probs_old, advantages [N, T, A, 1] (any shape of that many values); index: int64 [B] env-steps of
    the flattened [N T] (None: all).  `check_index` range-checks the index (one host synchronisation; skipped inside a graph capture).
    `workspace`: a uint8 device tensor of at least hns_actor_train_workspace_bytes bytes, 256-byte aligned, instead of one allocated per call;
    `out`: four fp32 device values that receive policy_loss, entropy, ess and grad_norm (the returned scalars are views of it) instead of a
    tensor of the call's own.  Both are ignored on the CPU."""
    if not clip_param >= 0:
        raise ValueError("clip_param must be >= 0")
    p = actor_parameters(actor)
    xs, xo, xc = _as_rollout(obs_self, obs_others, obs_cylinders)
    N, T, A, D_, K = _validate(p, xs, xo, xc, action, log_probs_old, advantages, index, check_index)
    if not xs.is_cuda:
        return _torch_loss_and_grad(p, xs, xo, xc, action, log_probs_old, advantages, index, float(clip_param), float(entropy_coef))
    dev = xs.device
    lib = abi.load_library()
    xs, xc = (t if t.stride(-1) == 1 else t.contiguous() for t in (xs, xc))
    if xo is not None and xo.stride(-1) != 1:
        xo = xo.contiguous()
    act, lpo, adv = action.contiguous(), log_probs_old.contiguous(), advantages.contiguous()
    B = index.numel() if index is not None else N * T
    net, grd = abi.HnsPolicyNet(), abi.HnsPolicyNet()
    for f, t in p.items():                                      # every refusal first: nothing is allocated for a call that is refused
        if t.data_ptr() % 16:
            raise ValueError(f"actor parameter {f} must be 16-byte aligned")
        if t.grad is not None and (t.grad.dtype != torch.float32 or not t.grad.is_contiguous() or t.grad.shape != t.shape or t.grad.device != dev):
            raise ValueError("existing .grad tensors must be contiguous float32 of the parameter's shape on its device")
    nbytes = lib.hns_actor_train_workspace_bytes(B * A, D_, A, K)
    if nbytes == 0:
        raise ValueError(f"shape outside the kernel's limits: {B * A} rows, self_dim {D_}, {A} agents, {K} cylinders")
    ws = _check_workspace(workspace, nbytes, dev) if workspace is not None else None
    scal = _check_out(out, 4, dev) if out is not None else None
    for f, t in p.items():
        if t.grad is None:
            t.grad = torch.empty_like(t)
        setattr(net, f, t.data_ptr())
        setattr(grd, f, t.grad.data_ptr())
    b = abi.HnsActorBatch()
    b.obs_self, b.obs_cylinders = xs.data_ptr(), xc.data_ptr()
    b.obs_others = xo.data_ptr() if xo is not None else None
    b.self_stride[:] = [xs.stride(0), xs.stride(1), xs.stride(2)]
    b.others_stride[:] = [xo.stride(0), xo.stride(1), xo.stride(2), xo.stride(3)] if xo is not None else [0, 0, 0, 0]
    b.cyl_stride[:] = [xc.stride(0), xc.stride(1), xc.stride(2), xc.stride(3)]
    b.num_envs, b.num_steps, b.batch = N, T, B
    b.index = index.data_ptr() if index is not None else None
    b.action, b.log_probs_old, b.advantages = act.data_ptr(), lpo.data_ptr(), adv.data_ptr()
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if scal is None:
        scal = torch.empty(4, dtype=torch.float32, device=dev)
    log_probs = torch.empty(B, A, 1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = lib.hns_actor_train_grad(C.byref(net), C.byref(b), D_, A, K, float(clip_param), float(entropy_coef), C.byref(grd), scal[0:].data_ptr(),
                                      scal[1:].data_ptr(), scal[2:].data_ptr(), scal[3:].data_ptr(), log_probs.data_ptr(), ws.data_ptr(), nbytes, st)
    _check(rc, "hns_actor_train_grad")
    return ActorLoss(scal[0], scal[1], scal[2], scal[3], log_probs)


def _actor_cfg(cfg):
    """The refusals of the actor's part of the algo cfg (policy.check_config's and critic_train's wording for the critic's counterparts)."""
    P.check_config(cfg)
    sget = _getter(_getter(cfg)("actor", None))
    if sget("lr_scheduler", None):
        raise P.PolicyConfigError("actor.lr_scheduler is not supported")
    if float(sget("weight_decay", 0.0) or 0.0) != 0:
        raise NotImplementedError("actor.weight_decay != 0 is not supported")
    return _getter(cfg), sget


def make_optimizer(actor, cfg=None):
    """The reference's actor_opt (mappo.py:154, :489) as a ClippedAdam: cfg is the algo cfg (actor.lr, actor.weight_decay, max_grad_norm)."""
    get, sget = _actor_cfg(cfg)
    return ClippedAdam(actor_parameters(actor).values(), lr=float(sget("lr", 5e-4)), max_grad_norm=get("max_grad_norm", 10.0),
                       weight_decay=float(sget("weight_decay", 0.0) or 0.0))


def update_actor(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, optimizer, index=None, cfg=None, check_index=False,
                 workspace=None, out=None):
    """MAPPOPolicy.update_actor on one minibatch: loss, backward, clip_grad_norm_, Adam.  cfg: the algo cfg (clip_param, entropy_coef; the
    reference's defaults when None).  Returns {"policy_loss", "actor_grad_norm", "entropy", "ESS"} as 0-dim tensors on the parameters' device
    — the caller decides when to .item().  `optimizer`: a ClippedAdam (make_optimizer).  The index is NOT range-checked by default, as in
    critic_train.update_critic.  `workspace`, `out`: policy_loss_and_grad's."""
    if not isinstance(optimizer, ClippedAdam):
        raise TypeError(f"update_actor takes a ClippedAdam (actor_train.make_optimizer), not {type(optimizer).__name__}: the clip and the "
                        "step are one launch that needs the gradient norm")
    get, _ = _actor_cfg(cfg)
    for group in optimizer.param_groups:
        if group.get("weight_decay", 0) != 0:
            raise NotImplementedError("weight_decay != 0 is not supported")
    res = policy_loss_and_grad(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, index,
                               clip_param=float(get("clip_param", 0.1)), entropy_coef=float(get("entropy_coef", 0.001)), check_index=check_index,
                               workspace=workspace, out=out)
    optimizer.step(grad_norm=res.grad_norm)
    norm = optimizer.last_grad_norm if getattr(optimizer, "last_grad_norm", None) is not None else res.grad_norm
    return {"policy_loss": res.policy_loss, "actor_grad_norm": norm, "entropy": res.entropy, "ESS": res.ess}
