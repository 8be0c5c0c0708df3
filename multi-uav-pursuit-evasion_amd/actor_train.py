"""The MAPPO actor's update on the device: MAPPOPolicy.update_actor (learning/mappo.py:271-324) for make_ppo_actor's network at
cfg/algo/mappo.yaml's defaults (share_actor, no tanh, no rnn, a 4-dim continuous action, DiagGaussian: fc_mean 128 -> 4 and a free log_std).

`policy_loss_and_grad(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, index)` is update_actor up to
`backward()`: device tensors go to ONE call of `hns_actor_train_grad` (one pass over the tiles: forward, log-probability, ratio, clipped
surrogate with its per-row backward weight, the encoder's backward pass; then the weight-gradient products and fixed-order sums) that fills
every parameter's `.grad` in its PyTorch layout and returns policy_loss, entropy, ESS and the total gradient norm as 0-dim device tensors —
no autograd graph, no host synchronisation.  `index` reads a minibatch of `make_dataset_naive` in place from the rollout's [N, T, A, ...]
tensors, as critic_train does.

The step is optim's `ClippedAdam` (clip_grad_norm_ + torch.optim.Adam in one call of `hns_adam_clipped`) over the actor's 23 tensors; it bumps the
parameters' version counters, so `policy.DevicePolicy` re-packs its operand image before the next forward pass.

With `global_rows=` the same calls are one rank's part of a data-parallel update: `hns_actor_train_grad_global` scales the rows
by 1 / global_rows and the entropy term by `entropy_share`, the gradients land in a `policy_train.GradBucket`, and with `group=` the bucket is
all-reduced and its norm taken before the step.

The `*_per_agent` functions are the same update with share_actor: False (one actor per agent: the reference's stacked `actor_params`, every
tensor [A, ...]; update_actor's else branch, mappo.py:288-291) on ONE call of `hns_actor_train_grad_agents`; DESIGN.md §7.16.  Their
data-parallel forms are `policy_loss_and_grad_per_agent_global` and `update_actor_per_agent_global` (`hns_actor_train_grad_agents_global`, the
bucket over the 23 stacked tensors).  All forms run ONE CPU function (`_torch_loss_and_grad`) and ONE device half
(`_device_loss_and_grad`, handed the entry and its workspace query).

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
from . import policy_train as PT
from .policy_train import ClippedAdam

ActorLoss = collections.namedtuple("ActorLoss", ["policy_loss", "entropy", "ess", "grad_norm", "log_probs"])


def actor_parameters(actor):
    """The actor's tensors by hns_policy_net field, in the order the parameters are registered (clip_grad_norm_'s order)."""
    return P.parse_parameters(actor, P.ACTOR_NAMES, "actor")


def _distribution(p, xs, xo, xc, action):
    """(log_probs_new, dist_entropy), [B, A, 1] each, of Actor.forward(eval_action=True) and DiagGaussian.forward (mappo.py:612-624,
    distributions.py:78-82) for the network `p` on rows of any leading shape; autograd through policy_train's encoder."""
    action_mean = F.linear(PT.encoder(p, xs, xo, xc), p["head_w"], p["head_b"])
    action_std = torch.broadcast_to(torch.exp(p["log_std"]), action_mean.shape)
    action_dist = D.Independent(D.Normal(action_mean, action_std, validate_args=False), 1, validate_args=False)
    return action_dist.log_prob(action).unsqueeze(-1), action_dist.entropy().unsqueeze(-1)


def _torch_loss_and_grad(p, xs, xo, xc, action, log_probs_old, advantages, index, clip_param, entropy_coef, global_rows=None, entropy_share=1.0,
                         group=None, bucket=None, per_agent=False):
    """update_actor's statements (mappo.py:293-318) on the gathered minibatch, behind the shared actor's `_distribution` or — `per_agent`,
    the else branch of mappo.py:288-291 — the actor mapped over dim 1 of its input and dim 0 of the stacked parameters, the outputs stacked
    on dim 1."""
    N, T, A, D_ = xs.shape
    xs, xc = xs.reshape(N * T, A, 1, D_), xc.reshape(N * T, A, xc.shape[3], 5)
    xo = xo.reshape(N * T, A, A - 1, 3) if xo is not None else None
    action = action.reshape(N * T, A, P.ACTION_DIM)
    log_probs_old, advantages = log_probs_old.reshape(N * T, A, 1), advantages.reshape(N * T, A, 1)
    if index is not None:
        xs, xc, action, log_probs_old, advantages = xs[index], xc[index], action[index], log_probs_old[index], advantages[index]
        xo = xo[index] if xo is not None else None
    leaves = {k: v.detach().requires_grad_(True) for k, v in p.items()}
    if per_agent:
        each = [_distribution(P.agent_slice(leaves, a), xs[:, a], xo[:, a] if xo is not None else None, xc[:, a], action[:, a]) for a in range(A)]
        log_probs_new, dist_entropy = (torch.stack(t, dim=1) for t in zip(*each))
    else:
        log_probs_new, dist_entropy = _distribution(leaves, xs, xo, xc, action)
    ratio = torch.exp(log_probs_new - log_probs_old)
    surr1 = ratio * advantages
    surr2 = torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param) * advantages
    entropy_loss = - torch.mean(dist_entropy)
    if global_rows is None:
        policy_loss = - torch.mean(torch.min(surr1, surr2) * P.ACTION_DIM)
        total = policy_loss + entropy_loss * entropy_coef
    else:                                                        # this rank's share of the union's mean; the entropy term counted once over the ranks
        policy_loss = - torch.sum(torch.min(surr1, surr2) * P.ACTION_DIM) / float(global_rows)
        total = policy_loss + entropy_loss * (entropy_coef * entropy_share)
    grads = torch.autograd.grad(total, list(leaves.values()))
    for t, g in zip(p.values(), grads):
        t.grad = g
    with torch.no_grad():
        if global_rows is None:
            grad_norm = nn.utils.clip_grad_norm_(list(p.values()), float("inf"))      # the total norm as clip_grad_norm_ forms it; scales by 1
        else:
            if bucket is not None:
                bucket.adopt()
            grad_norm = PT.finish_global(bucket, group)
        ess = (2 * ratio.logsumexp(0) - (2 * ratio).logsumexp(0)).exp().mean() / ratio.shape[0]
        entropy = -entropy_loss.detach()
        if per_agent and global_rows is not None:
            # The same on every rank: the fp32 mean over the rows above rounds differently for different row counts once the agents' entropies
            # differ, so the global form states what hns_actor_train_grad_agents_global computes — each agent's four terms and the mean over the
            # agents in fp64, rounded once.  It is the row mean's value up to that mean's own summation error.
            ls = p["log_std"].detach()
            entropy = (0.5 + 0.9189385332046727 + ls.double()).sum(-1).mean().to(ls.dtype)
    return ActorLoss(policy_loss.detach(), entropy, ess, grad_norm, log_probs_new.detach())


def _device_loss_and_grad(entry, workspace_bytes, p, xs, xo, xc, shape, action, log_probs_old, advantages, index, clip_param, entropy_coef, workspace,
                          out, more=()):
    """The device half of both `policy_loss_and_grad`s: ONE call of `entry` — hns_actor_train_grad, or its _agents or _global form, with its
    workspace query, both taken from the library — on validated device tensors.  `more`: the global form's arguments behind the stream;
    with them the entry leaves grad_norm to the caller.  Returns (the four result slots, log_probs [B, A, 1])."""
    act, lpo, adv = action.contiguous(), log_probs_old.contiguous(), advantages.contiguous()
    net, grd, b, ws, nbytes, scal, B, st = PT.prepare_call("actor", p, xs, xo, xc, index, shape, workspace_bytes, workspace, out, 4, abi.HnsActorBatch)
    _, _, A, D_, K = shape
    b.action, b.log_probs_old, b.advantages = act.data_ptr(), lpo.data_ptr(), adv.data_ptr()
    log_probs = torch.empty(B, A, 1, dtype=torch.float32, device=xs.device)
    with torch.cuda.device(xs.device):
        rc = entry(C.byref(net), C.byref(b), D_, A, K, float(clip_param), float(entropy_coef), C.byref(grd), scal[0:].data_ptr(), scal[1:].data_ptr(),
                   scal[2:].data_ptr(), None if more else scal[3:].data_ptr(), log_probs.data_ptr(), ws.data_ptr(), nbytes, st, *more)
    abi.check(rc, entry.__name__)
    return scal, log_probs


def policy_loss_and_grad(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, index=None, clip_param=0.1,
                         entropy_coef=0.001, check_index=True, workspace=None, out=None, global_rows=None, entropy_share=1.0, group=None, bucket=None):
    """The clipped PPO surrogate of the actor on a minibatch (plus entropy_coef times the entropy loss) and every parameter's .grad (as
    zero_grad() + backward() leave them, before clip_grad_norm_).  Returns ActorLoss(policy_loss, entropy, ess, grad_norm: 0-dim tensors;
    log_probs [B, A, 1]: the new log-probabilities of the stored actions).

    obs_*: the rollout's [N, T, A, ...] observations or a flat [R, A, ...] batch, read in place (critic_train.value_loss_and_grad's
    layouts); action [N, T, A, 4], log_probs_old, advantages [N, T, A, 1] (any shape of that many values); index: int64 [B] env-steps of
    the flattened [N T] (None: all).  `check_index` range-checks the index (one host synchronisation; skipped inside a graph capture).
    `workspace`: a uint8 device tensor of at least hns_actor_train_workspace_bytes bytes, 256-byte aligned, instead of one allocated per call;
    `out`: four fp32 device values that receive policy_loss, entropy, ess and grad_norm (the returned scalars are views of it) instead of a
    tensor of the call's own.  Both are ignored on the CPU.

    `global_rows` (None: the call above, untouched): this minibatch is one rank's part of a union of `global_rows` agent rows
    (hns_actor_train_grad_global).  policy_loss is then this rank's SHARE, -4 sum_local / global_rows, and the gradients are the share's: over
    the ranks both add up to the union's.  `entropy_share`: the part of the entropy term's gradient this rank adds (1 / world).  ess stays
    this rank's own.  `bucket`: the actor's `policy_train.GradBucket`; grad_norm is then the norm of the bucket (None without one).
    `group`: the bucket is all-reduced (SUM) over it first, so the gradients and grad_norm are the union's, the same on every rank."""
    if not clip_param >= 0:
        raise ValueError("clip_param must be >= 0")
    p = actor_parameters(actor)
    xs, xo, xc = PT.as_rollout(obs_self, obs_others, obs_cylinders)
    shape = PT.validate("actor", p, xs, xo, xc, (("action", action, P.ACTION_DIM), ("log_probs_old", log_probs_old, 1),
                                                 ("advantages", advantages, 1)), index, check_index)
    B = index.numel() if index is not None else shape[0] * shape[1]
    PT.check_global("actor", p, global_rows, B * shape[2], group, bucket)
    if not xs.is_cuda:
        return _torch_loss_and_grad(p, xs, xo, xc, action, log_probs_old, advantages, index, float(clip_param), float(entropy_coef), global_rows,
                                    float(entropy_share), group, bucket)
    lib = abi.load_library()
    args = (lib.hns_actor_train_workspace_bytes, p, xs, xo, xc, shape, action, log_probs_old, advantages, index, clip_param, entropy_coef, workspace, out)
    if global_rows is not None:
        scal, log_probs = _device_loss_and_grad(lib.hns_actor_train_grad_global, *args, more=(int(global_rows), float(entropy_share)))
        norm = PT.finish_global(bucket, group, scal[3:4])
        return ActorLoss(scal[0], scal[1], scal[2], scal[3] if norm is not None else None, log_probs)
    scal, log_probs = _device_loss_and_grad(lib.hns_actor_train_grad, *args)
    return ActorLoss(scal[0], scal[1], scal[2], scal[3], log_probs)


def actor_cfg(cfg, per_agent=False):
    """The refusals of the actor's part of the algo cfg (policy.check_config's — `per_agent`: check_config_per_agent's — then
    actor.lr_scheduler, actor.weight_decay); returns the cfg's and the actor section's getters."""
    (P.check_config_per_agent if per_agent else P.check_config)(cfg)
    sget = PT.getter(PT.getter(cfg)("actor", None))
    if sget("lr_scheduler", None):
        raise P.PolicyConfigError("actor.lr_scheduler is not supported")
    if float(sget("weight_decay", 0.0) or 0.0) != 0:
        raise NotImplementedError("actor.weight_decay != 0 is not supported")
    return PT.getter(cfg), sget


def make_optimizer(actor, cfg=None, per_agent=False):
    """The reference's actor_opt (mappo.py:154, :489) as a ClippedAdam: cfg is the algo cfg (actor.lr, actor.weight_decay, max_grad_norm).
    `per_agent`: over the 23 STACKED tensors — ONE Adam and one clip over all agents' parameters, as the reference's."""
    get, sget = actor_cfg(cfg, per_agent)
    return ClippedAdam((actor_parameters_per_agent if per_agent else actor_parameters)(actor).values(), lr=float(sget("lr", 5e-4)),
                       max_grad_norm=get("max_grad_norm", 10.0), weight_decay=float(sget("weight_decay", 0.0) or 0.0))


def _info(res, norm):
    return {"policy_loss": res.policy_loss, "actor_grad_norm": norm, "entropy": res.entropy, "ESS": res.ess}


def update_actor(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, optimizer, index=None, cfg=None, check_index=False,
                 workspace=None, out=None, global_rows=None, entropy_share=1.0, group=None, bucket=None):
    """MAPPOPolicy.update_actor on one minibatch: loss, backward, clip_grad_norm_, Adam.  cfg: the algo cfg (clip_param, entropy_coef; the
    reference's defaults when None).  Returns {"policy_loss", "actor_grad_norm", "entropy", "ESS"} as 0-dim tensors on the parameters' device
    — the caller decides when to .item().  `optimizer`: a ClippedAdam (make_optimizer).  The index is NOT range-checked by default, as in
    critic_train.update_critic.  `workspace`, `out`: policy_loss_and_grad's.  `global_rows`, `entropy_share`, `group`, `bucket`:
    policy_loss_and_grad's — one rank's part of a data-parallel update; the step needs the union's gradients, so all four travel together
    (group may be None where the caller summed the buckets itself)."""
    if global_rows is not None and bucket is None:
        raise ValueError("update_actor with global_rows= steps on the bucket's norm: pass bucket=")
    get, _ = PT.check_optimizer(optimizer, "update_actor", "actor_train.make_optimizer", actor_cfg, cfg)
    res = policy_loss_and_grad(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, index,
                               clip_param=float(get("clip_param", 0.1)), entropy_coef=float(get("entropy_coef", 0.001)), check_index=check_index,
                               workspace=workspace, out=out, global_rows=global_rows, entropy_share=entropy_share, group=group, bucket=bucket)
    return _info(res, PT.clipped_step(optimizer, res.grad_norm))


# ---------------------------------------------------------------------------------------------------------------------------------------
# one actor per agent (share_actor: False)
def actor_parameters_per_agent(actor):
    """The STACKED actor's tensors ([A, ...] each) by hns_policy_net field, in registration order (clip_grad_norm_'s: the reference clips the
    stacked tensors)."""
    return P.parse_parameters_per_agent(actor, "actor")[0]


def _loss_and_grad_per_agent(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, index, clip_param, entropy_coef, check_index,
                             workspace, out, global_rows=None, entropy_share=1.0, group=None, bucket=None):
    """Both per-agent `policy_loss_and_grad`s: the local call (global_rows None: hns_actor_train_grad_agents) and one rank's part of a
    data-parallel update (hns_actor_train_grad_agents_global, then policy_train.finish_global on the bucket)."""
    if not clip_param >= 0:
        raise ValueError("clip_param must be >= 0")
    p = actor_parameters_per_agent(actor)
    for k, t in p.items():
        if not t.is_contiguous():
            raise ValueError(f"actor parameter {k} must be contiguous")
    xs, xo, xc = PT.as_rollout(obs_self, obs_others, obs_cylinders)
    shape = PT.validate("actor", P.agent_slice(p, 0), xs, xo, xc, (("action", action, P.ACTION_DIM), ("log_probs_old", log_probs_old, 1),
                                                                   ("advantages", advantages, 1)), index, check_index)
    A = int(p["in_proj_w"].shape[0])
    if shape[2] != A:
        raise ValueError(f"the observation has {shape[2]} agents, the stacked actor {A}")
    B = index.numel() if index is not None else shape[0] * shape[1]
    PT.check_global("actor", p, global_rows, B * A, group, bucket)
    if not xs.is_cuda:
        return _torch_loss_and_grad(p, xs, xo, xc, action, log_probs_old, advantages, index, float(clip_param), float(entropy_coef), global_rows,
                                    float(entropy_share), group, bucket, per_agent=True)
    lib = abi.load_library()
    args = (lib.hns_actor_train_agents_workspace_bytes, p, xs, xo, xc, shape, action, log_probs_old, advantages, index, clip_param, entropy_coef, workspace,
            out)
    if global_rows is not None:
        scal, log_probs = _device_loss_and_grad(lib.hns_actor_train_grad_agents_global, *args, more=(int(global_rows), float(entropy_share)))
        norm = PT.finish_global(bucket, group, scal[3:4])
        return ActorLoss(scal[0], scal[1], scal[2], scal[3] if norm is not None else None, log_probs)
    scal, log_probs = _device_loss_and_grad(lib.hns_actor_train_grad_agents, *args)
    return ActorLoss(scal[0], scal[1], scal[2], scal[3], log_probs)


def policy_loss_and_grad_per_agent(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, index=None, clip_param=0.1,
                                   entropy_coef=0.001, check_index=True, workspace=None, out=None):
    """`policy_loss_and_grad` with one actor per agent: `actor` holds the STACKED tensors ([A, ...], the reference's actor_params with
    share_actor: False), agent a's rows run on slice a, and every stacked tensor's .grad ([A, ...]) is as zero_grad() + backward() leave it.
    policy_loss is the mean over all B A rows, entropy the mean over the agents of each agent's entropy (each d log_std takes
    -entropy_coef / A), ess as for the shared actor, grad_norm the total norm over all agents' gradients.  Arguments, layouts, `workspace`
    (at least hns_actor_train_agents_workspace_bytes bytes) and `out` as `policy_loss_and_grad`; the data-parallel form is
    `policy_loss_and_grad_per_agent_global`.  log_probs [B, A, 1] is bit for bit `policy_loss_and_grad`'s for row (b, a) with slice a as the
    shared actor."""
    return _loss_and_grad_per_agent(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, index, clip_param, entropy_coef,
                                    check_index, workspace, out)


def policy_loss_and_grad_per_agent_global(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, index=None, clip_param=0.1,
                                          entropy_coef=0.001, check_index=True, workspace=None, out=None, global_rows=None, entropy_share=1.0,
                                          group=None, bucket=None):
    """`policy_loss_and_grad_per_agent` as one rank's part of a data-parallel update (hns_actor_train_grad_agents_global),
    with the semantics of `policy_loss_and_grad(global_rows=...)`: this minibatch is a part of a union of `global_rows` agent rows, policy_loss
    is this rank's SHARE (-4 sum_local / global_rows), every stacked gradient is the share's, each agent's d log_std takes
    (-entropy_coef entropy_share) / A, entropy is the same on every rank and ess stays this rank's own.  `bucket`: the `policy_train.GradBucket`
    of the 23 stacked tensors; grad_norm is the bucket's norm (None without one).  `group`: the bucket is all-reduced (SUM) over it first.
    With global_rows = this call's own rows and entropy_share 1 every output has `policy_loss_and_grad_per_agent`'s bits."""
    if global_rows is None:
        raise ValueError("policy_loss_and_grad_per_agent_global needs global_rows= (the local call is policy_loss_and_grad_per_agent)")
    return _loss_and_grad_per_agent(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, index, clip_param, entropy_coef,
                                    check_index, workspace, out, global_rows, entropy_share, group, bucket)


def actor_cfg_per_agent(cfg):
    """`actor_cfg` for one actor per agent: policy.check_config_per_agent's refusals, then actor.lr_scheduler and actor.weight_decay."""
    return actor_cfg(cfg, per_agent=True)


def make_optimizer_per_agent(actor, cfg=None):
    """`make_optimizer` over the 23 STACKED tensors: ONE Adam and one clip over all agents' parameters, as the reference's actor_opt."""
    return make_optimizer(actor, cfg, per_agent=True)


def update_actor_per_agent(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, optimizer, index=None, cfg=None,
                           check_index=False, workspace=None, out=None):
    """`update_actor` with one actor per agent (MAPPOPolicy.update_actor with share_actor: False): `policy_loss_and_grad_per_agent`, then the
    clip and the Adam step of `optimizer` (make_optimizer_per_agent) over the stacked tensors.  The same info dict."""
    get, _ = PT.check_optimizer(optimizer, "update_actor_per_agent", "actor_train.make_optimizer_per_agent", actor_cfg_per_agent, cfg)
    res = policy_loss_and_grad_per_agent(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, index,
                                         clip_param=float(get("clip_param", 0.1)), entropy_coef=float(get("entropy_coef", 0.001)),
                                         check_index=check_index, workspace=workspace, out=out)
    return _info(res, PT.clipped_step(optimizer, res.grad_norm))


def update_actor_per_agent_global(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, optimizer, index=None, cfg=None,
                                  check_index=False, workspace=None, out=None, global_rows=None, entropy_share=1.0, group=None, bucket=None):
    """`update_actor_per_agent` as one rank's part of a data-parallel update: `policy_loss_and_grad_per_agent_global`, then the clip by the
    bucket's norm and the Adam step over the stacked tensors.  The step needs the union's gradients, so `global_rows` and `bucket` are
    required (`group` may be None where the caller summed the buckets itself), as `update_actor(global_rows=...)`."""
    if global_rows is None or bucket is None:
        raise ValueError("update_actor_per_agent_global steps on the bucket's norm over the union: pass global_rows= and bucket=")
    get, _ = PT.check_optimizer(optimizer, "update_actor_per_agent_global", "actor_train.make_optimizer_per_agent", actor_cfg_per_agent, cfg)
    res = policy_loss_and_grad_per_agent_global(actor, obs_self, obs_others, obs_cylinders, action, log_probs_old, advantages, index,
                                                clip_param=float(get("clip_param", 0.1)), entropy_coef=float(get("entropy_coef", 0.001)),
                                                check_index=check_index, workspace=workspace, out=out, global_rows=global_rows,
                                                entropy_share=entropy_share, group=group, bucket=bucket)
    return _info(res, PT.clipped_step(optimizer, res.grad_norm))
