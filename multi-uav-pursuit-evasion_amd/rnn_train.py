"""One recurrent MAPPO update per network on the device: MAPPOPolicy.update_actor / update_critic (learning/mappo.py:271-352) for the
`actor.rnn` / `critic.rnn` configuration — encoder -> GRU -> head — over the stored sequences of a rollout.

A minibatch is B (env, segment) pairs of L = train_seq_len steps: segment id s of the flattened [N, T / L] starts from its STORED state and
re-runs its L steps under the stored env-level `is_init` flags, so the recomputed log-probabilities are the collected ones up to rounding.
`update_actor_rnn` / `update_critic_rnn` run, on one stream and without a host synchronisation:

    encoder.device_forward     index = segment L + t in [B, L] order: the [B L A, 128] features ARE the GRU's [B, A, L, 128] view
    rnn.device_forward         from the gathered stored state and the flags of the segment's steps, keeping h_hist
    hns_rnn_*_head_grad        the head, the distribution / value loss and their backward pass down to dy (csrc/hns_rnn_train.hip)
    rnn.device_backward        dout = dy, no dh_last; dx lands in the encoder op's row order
    encoder.device_backward    dfeatures = dx: the same memory, no permute copy
    GradBucket.norm            ONE flat bucket: the encoder's 20 tensors, the GRU's 6 and the head's, in the optimiser's order
    ClippedAdam.step           clip_grad_norm_ + Adam in one launch

`policy_loss_and_grad_rnn` / `value_loss_and_grad_rnn` are the same calls up to the norm, as actor_train.policy_loss_and_grad is to
update_actor; with `value_loss_sums_rnn` they are the three callers of ONE path (`_run`), which a `_Head` — the C call, its restatement, its
per-row tensors and result keys — is all that tells apart.  `RnnWorkspace` keeps every buffer of a call between calls (the learner holds one per network).

With `global_rows=` the same calls are one rank's part of a data-parallel update over the union of the ranks' minibatches, as
in actor_train / critic_train: only the head entries take their global forms (`hns_rnn_actor_head_grad_global`; `hns_rnn_critic_head_sums`, the
SUM all-reduce of five fp64 values, `hns_rnn_critic_head_grad_global`) — everything behind dy is linear in it — and the bucket is all-reduced
before its norm is taken.  `value_loss_sums_rnn` is the critic's forward half; its forward state lets `value_loss_and_grad_rnn(forward=)` go on
from y without a second encoder and GRU pass.

The `*_per_agent` functions are the actor's update with share_actor: False (one actor AND one actor GRU per agent: the reference's stacked
`actor_params`, every tensor [A, ...]) through the SAME path: the encoder op and the GRU op take the stacked tensors
(`hns_encoder_*_agents`, `hns_gru_*_agents`), the head entry is `hns_rnn_actor_head_grad_agents`, and ONE bucket, ONE norm and ONE ClippedAdam
step run over the 29 stacked tensors.  The critic stays shared: `update_critic_rnn`, untouched.  Their data-parallel forms are
`policy_loss_and_grad_rnn_per_agent_global` / `update_actor_rnn_per_agent_global` (`hns_rnn_actor_head_grad_agents_global`, the bucket over the
29 stacked tensors).

CPU tensors run the same statements in torch: `policy_train.encoder`, `rnn.restatement`, and `actor_head` / `critic_head` — the head and the
loss written out with their hand-derived dy (what the kernels compute, not autograd of another formula); the encoder's and the GRU's
gradients come from autograd over the recomputed restatements, as in `encoder.encode` and `rnn.gru` (tests — not the hot path)."""
import collections
import ctypes as C
import math

import torch

from . import abi, actor_train, critic_train, encoder
from . import policy as P
from . import policy_train as PT
from . import rnn
from .policy_train import ClippedAdam

H = abi.HNS_GRU_HIDDEN
LOG_SQRT_2PI = 0.9189385332046727
ActorLoss, CriticLoss = actor_train.ActorLoss, critic_train.CriticLoss
CriticSumsRnn = collections.namedtuple("CriticSumsRnn", ["sums", "values", "forward"])
Network = collections.namedtuple("Network", ["encoder", "gru", "head"])        # three {field: tensor} mappings of one network


def network_parameters(network, actor, stacked=False):
    """Network(encoder, gru, head) of a recurrent actor (`actor` true) or critic from the reference's names, as RecurrentDevicePolicy parses
    them: the encoder's tensors by hns_policy_net field in encoder.FIELDS' order, the GRU's six by hns_gru_net field, the head's (head_w,
    head_b and the actor's log_std).  Their concatenation in this order is the optimiser's and the gradient bucket's order.  stacked (one
    actor per agent, as PerAgentRecurrentDevicePolicy parses it): every tensor [A, ...] with one A."""
    word = "actor" if actor else "critic"
    if stacked:
        if not actor:
            raise P.PolicyConfigError("critic: the critic is shared; only the actor's tensors are stacked over the agents")
        rest, gru, A_rnn = P.split_rnn(network, word, stacked=True)
        p, A = P.parse_parameters(rest, P.ACTOR_NAMES, word, stacked=True)
        if A != A_rnn:
            raise P.PolicyConfigError(f"actor: {A} stacked actors with {A_rnn} stacked GRUs")
    else:
        rest, gru = P.split_rnn(network, word)
        p = P.parse_parameters(rest, P.ACTOR_NAMES if actor else P.CRITIC_NAMES, word)
    enc = encoder.encoder_parameters({f: p[f] for f in encoder.FIELDS if f in p}, stacked)
    head = {f: p[f] for f in ("head_w", "head_b") + (("log_std",) if actor else ())}
    return Network(enc, gru, head)


def flat_parameters(net):
    return [*net.encoder.values(), *net.gru.values(), *net.head.values()]


def make_optimizer(network, cfg=None, actor=True, stacked=False):
    """The reference's actor_opt / critic_opt over ALL of a recurrent network's tensors (encoder, rnn, head) as a ClippedAdam: cfg is the
    algo cfg (actor.lr / critic.lr, max_grad_norm); the refusals are actor_train.actor_cfg's / critic_train.critic_cfg's without the rnn one
    (`stacked`: actor_cfg_per_agent's — share_actor must be False)."""
    sub = PT.getter(PT.getter(cfg)("actor" if actor else "critic", None))
    rest = P.cfg_without(cfg, "actor.rnn", "critic.rnn")
    if actor:
        actor_train.actor_cfg(rest, per_agent=stacked)
    else:
        critic_train.critic_cfg(rest)
    return ClippedAdam(flat_parameters(network_parameters(network, actor, stacked)), lr=float(sub("lr", 5e-4)),
                       max_grad_norm=PT.getter(cfg)("max_grad_norm", 10.0))


def make_optimizer_per_agent(actor, cfg=None):
    """`make_optimizer` over the 29 STACKED tensors of one recurrent actor per agent: ONE Adam and one clip over all agents' parameters, as the
    reference's actor_opt."""
    return make_optimizer(actor, cfg, actor=True, stacked=True)


# ---- the head and the loss, restated: any dtype (the tests run them in fp64 against autograd of the reference's statements)
def actor_head(head_w, head_b, log_std, y, action, log_probs_old, advantages, clip_param, entropy_coef, global_rows=None, entropy_share=1.0):
    """hns_rnn_actor_head_grad's statements on gathered rows: y [B, L, A, 128], action [B, L, A, 4], log_probs_old / advantages [B, L, A].
    Returns a dict: dy [B, L, A, 128], d_head_w, d_head_b, d_log_std, policy_loss, entropy, ess (0-dim), log_probs [B, L, A].
    `global_rows`: hns_rnn_actor_head_grad_global's — every mean divides by the union's row count, policy_loss is this part's share and
    d_log_std takes `entropy_share` of the entropy term's constant gradient; ess stays the part's own.
    One head per agent (hns_rnn_actor_head_grad_agents): head_w [A, 4, 128], head_b / log_std [A, 4] — row (b, t, a) runs on slice a, the
    gradients are stacked the same way, entropy is the mean over the agents of each agent's and every d_log_std[a] takes -entropy_coef / A
    (with `global_rows`, hns_rnn_actor_head_grad_agents_global's: -(entropy_coef entropy_share) / A, and every mean over the union)."""
    B = y.shape[0]
    n = float(y.shape[0] * y.shape[1] * y.shape[2]) if global_rows is None else float(global_rows)
    per_agent = head_w.dim() == 3
    mu = torch.einsum("blah,aoh->blao", y, head_w) + head_b if per_agent else y @ head_w.t() + head_b
    # logp is formed in fp64 from the fp32 mean (its rounding is the ratio's relative error), as the kernel forms it
    iv64 = torch.exp(-2.0 * log_std.double())
    dm64 = action.double() - mu.double()
    z64 = dm64 * dm64 * iv64
    logp64 = ((-0.5 * z64 - log_std.double()) - LOG_SQRT_2PI).sum(-1)
    z2, logp = z64.to(y.dtype), logp64.to(y.dtype)
    ratio = torch.exp((logp64 - log_probs_old.double()).to(y.dtype))
    lo, hi = 1.0 - clip_param, 1.0 + clip_param
    s1, s2 = ratio * advantages, ratio.clamp(lo, hi) * advantages
    inside = (ratio >= lo) & (ratio <= hi)
    wgt = (inside | (s1 < s2)).to(y.dtype)                       # min's and clamp's backward weight, per row
    dlogp = (-float(P.ACTION_DIM) * advantages * ratio * wgt / n).unsqueeze(-1)
    dmu = dlogp * (dm64 * iv64).to(y.dtype)
    flat = lambda t: t.reshape(-1, t.shape[-1])                  # noqa: E731
    ess = (2 * ratio.logsumexp(0) - (2 * ratio).logsumexp(0)).exp().mean() / B
    if per_agent:
        A = head_w.shape[0]
        return {"dy": torch.einsum("blao,aoh->blah", dmu, head_w), "d_head_w": torch.einsum("blao,blah->aoh", dmu, y), "d_head_b": dmu.sum((0, 1)),
                "d_log_std": (dlogp * (z2 - 1.0)).sum((0, 1)) - (entropy_coef if global_rows is None else entropy_coef * entropy_share) / A,
                "policy_loss": -float(P.ACTION_DIM) * (torch.minimum(s1, s2).mean() if global_rows is None else torch.minimum(s1, s2).sum() / n),
                "entropy": (0.5 + LOG_SQRT_2PI + log_std).sum(-1).mean(), "ess": ess, "log_probs": logp}
    return {"dy": dmu @ head_w, "d_head_w": flat(dmu).t() @ flat(y), "d_head_b": flat(dmu).sum(0),
            "d_log_std": flat(dlogp * (z2 - 1.0)).sum(0) - (entropy_coef if global_rows is None else entropy_coef * entropy_share),
            "policy_loss": -float(P.ACTION_DIM) * (torch.minimum(s1, s2).mean() if global_rows is None else torch.minimum(s1, s2).sum() / n), "entropy": (0.5 + LOG_SQRT_2PI + log_std).sum(), "ess": ess,
            "log_probs": logp}


def critic_head_sums(head_w, head_b, y, b_values, b_returns, clip_param, loss="huber", huber_delta=10.0):
    """hns_rnn_critic_head_sums' statements on gathered rows: (the five fp64 sums of these rows, values [B, L, A])."""
    v = (y @ head_w.t() + head_b).squeeze(-1)
    clipped = b_values + (v - b_values).clamp(-clip_param, clip_param)
    e0, e1, r64 = (v - b_returns).double(), (clipped - b_returns).double(), b_returns.double()
    lossf = lambda x: x * x if loss == "mse" else torch.where(x.abs() < huber_delta, 0.5 * x * x, huber_delta * (x.abs() - 0.5 * huber_delta))   # noqa: E731
    return torch.stack([lossf(e0).sum(), lossf(e1).sum(), (e0 ** 2).sum(), r64.sum(), (r64 * r64).sum()]), v


def critic_head(head_w, head_b, y, b_values, b_returns, clip_param, loss="huber", huber_delta=10.0, sums=None, global_rows=None):
    """hns_rnn_critic_head_grad's statements on gathered rows: y [B, L, A, 128], b_values / b_returns [B, L, A].  Returns a dict: dy,
    d_head_w [1, 128], d_head_b [1], value_loss, explained_var (0-dim), values [B, L, A].  `sums`, `global_rows`:
    hns_rnn_critic_head_grad_global's — the decision, value_loss and explained_var from the union's five sums over global_rows, dv over
    global_rows."""
    n = float(b_values.numel()) if global_rows is None else float(global_rows)
    v = (y @ head_w.t() + head_b).squeeze(-1)
    d = v - b_values
    clipped = b_values + d.clamp(-clip_param, clip_param)

    def lossf(x):
        return x * x if loss == "mse" else torch.where(x.abs() < huber_delta, 0.5 * x * x, huber_delta * (x.abs() - 0.5 * huber_delta))

    def dloss(x):
        return 2.0 * x if loss == "mse" else x.clamp(-huber_delta, huber_delta)

    e0, e1 = v - b_returns, clipped - b_returns
    if sums is not None:
        S = sums.double()
        lo, lc = S[0] / n, S[1] / n
    else:
        lo, lc = lossf(e0.double()).sum() / n, lossf(e1.double()).sum() / n
    w0, w1 = (1.0, 0.0) if lo > lc else ((0.0, 1.0) if lo < lc else (0.5, 0.5))      # the max of two means: one branch, halves at a tie
    inside = ((d >= -clip_param) & (d <= clip_param)).to(y.dtype)
    dv = ((w0 * dloss(e0) + w1 * dloss(e1) * inside) / n).unsqueeze(-1)
    r64 = b_returns.double()
    if sums is not None:
        var, mse = (S[4] - S[3] * S[3] / n) / (n - 1.0), S[2] / n
    else:
        var, mse = ((r64 * r64).sum() - r64.sum() ** 2 / n) / (n - 1.0), (e0.double() ** 2).sum() / n
    return {"dy": dv * head_w.reshape(-1), "d_head_w": (dv * y).reshape(-1, y.shape[-1]).sum(0, keepdim=True), "d_head_b": dv.sum().reshape(1),
            "value_loss": torch.maximum(lo, lc).to(y.dtype), "explained_var": (1.0 - mse / var).to(y.dtype), "values": v}


# ---- buffers kept between calls
class RnnWorkspace:
    """Every buffer of an update call, kept between calls and regrown only when a shape grows: the features, y, h_hist, dy, dx, h_last and
    the three kernels' workspaces.  One per network (the learner holds two)."""

    def __init__(self):
        self._t = {}

    def get(self, name, numel, dtype, device):
        t = self._t.get(name)
        if t is None or t.numel() < numel or t.device != device or t.dtype != dtype:
            t = self._t[name] = torch.empty(max(int(numel), 1), dtype=dtype, device=device)
            if t.data_ptr() % 256:
                raise RuntimeError("the allocator returned a buffer that is not 256-byte aligned")
        return t

    def floats(self, name, shape, device):
        return self.get(name, math.prod(shape), torch.float32, device)[:math.prod(shape)].view(shape)

    def bytes(self, name, nbytes, device):
        return self.get(name, nbytes, torch.uint8, device)

    def release(self):
        self._t = {}


def make_bucket(network, actor, stacked=False):
    """The gradient bucket of a recurrent network for `bucket=`: ONE flat buffer behind the .grad of the encoder's, the GRU's and the head's
    tensors (`stacked`: the 29 stacked tensors of one actor per agent), in network_parameters' order.  A caller that makes many calls keeps
    one (the learner does); a call without one makes its own."""
    return PT.GradBucket(flat_parameters(network_parameters(network, actor, stacked)))


def _bucket(net, bucket):
    """The call's gradient bucket: the caller's, checked, or a new one."""
    params = flat_parameters(net)
    if bucket is None:
        return PT.GradBucket(params)
    if not isinstance(bucket, PT.GradBucket) or len(bucket.params) != len(params) or any(a is not b for a, b in zip(bucket.params, params)):
        raise ValueError("bucket= must be the GradBucket of this network's parameters in network_parameters' order (make_bucket)")
    if bucket.flat.is_cuda and not bucket.owns(params):
        raise ValueError("a parameter's .grad no longer lies in bucket=")
    return bucket


def _prepare(word, net, obs, state, is_init, per_row, segment, seq_len, check_index):
    """The checks every entry shares; returns (xs, xo, xc, shape, segment ids [B], L, segments in the rollout)."""
    xs, xo, xc = PT.as_rollout(*obs)
    agents = encoder.stacked_agents(net.encoder)
    shape = PT.validate(word, net.encoder if agents is None else P.agent_slice(net.encoder, 0), xs, xo, xc, per_row, None, False)
    N, T, A, _, _ = shape
    if agents is not None and agents != A:
        raise ValueError(f"the observation has {A} agents, the stacked {word} {agents}")
    L = int(seq_len)
    if not 1 <= L <= abi.HNS_GRU_MAX_STEPS or T % L:
        raise ValueError(f"the segment length {L} must be in [1, {abi.HNS_GRU_MAX_STEPS}] and divide the rollout's {T} steps")
    NS = N * (T // L)
    dev = xs.device
    if not torch.is_tensor(state) or state.dtype != torch.float32 or state.numel() != NS * A * H or state.shape[-1] != H or state.device != dev:
        raise ValueError(f"the stored state must be float32 [{N}, {T // L}, {A}, {H}] on {dev}")
    if not torch.is_tensor(is_init) or is_init.numel() != N * T or is_init.device != dev:
        raise ValueError(f"is_init must hold [{N}, {T}, 1] flags on {dev}")
    for f, t in (*net.gru.items(), *net.head.items()):
        if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{word} parameter {f} must be a contiguous float32 tensor on {dev}")
    if segment is None:
        segment = torch.arange(NS, device=dev)
    else:
        if not torch.is_tensor(segment) or segment.dtype != torch.int64 or segment.dim() != 1 or segment.device != dev:
            raise TypeError(f"segment must be a 1-d int64 tensor on {dev}")
        if segment.numel() < 1:
            raise ValueError("empty minibatch: the mean over zero rows is NaN")
        segment = segment.contiguous()
        if check_index and not (dev.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            lo, hi = torch.stack([segment.min(), segment.max()]).tolist()        # one host synchronisation
            if lo < 0 or hi >= NS:
                raise IndexError(f"segment ids [{lo}, {hi}] outside the {NS} segments of the rollout")
    return xs, xo, xc, shape, segment, L, NS


def _gathered(state, is_init, segment, NS, A, L):
    """(h0 [B A, 128], flags uint8 [B A, L]) of the minibatch: the stored state going into each segment and the env-level flags of its steps
    for every agent, from clamped ids (_device_forward_to_y)."""
    seg = segment.clamp(0, NS - 1)
    B = seg.numel()
    h0 = state.reshape(NS, A, H).index_select(0, seg).reshape(B * A, H)
    f = is_init.reshape(NS, L)
    f = f.view(torch.uint8) if f.dtype == torch.bool else (f != 0).view(torch.uint8)
    # (contiguous(): for B = 1 the reshape of the expanded [1, A, L] is a VIEW with stride 0 over the agents, which the kernels, reading
    # flags[s L + t], would take for A L bytes: the agents past the first read behind the segment's L flags)
    flags = f.index_select(0, seg).unsqueeze(1).expand(B, A, L).reshape(B * A, L).contiguous()
    return h0, flags


def _step_index(segment, L):
    """The env-steps of the segments, in [B, L] order: segment L + t."""
    return (segment.unsqueeze(1) * L + torch.arange(L, device=segment.device)).reshape(-1)


def _rows(per_row, segment, L, A):
    """Per-row tensors of the rollout ([N T, A(, k)] values) gathered as [B, L, A(, k)]."""
    idx = _step_index(segment, L)
    out = []
    for t, width in per_row:
        t = t.reshape(-1, A, width) if width > 1 else t.reshape(-1, A)
        out.append(t.index_select(0, idx).reshape(segment.numel(), L, *t.shape[1:]))
    return idx, out


def _torch_forward(net, xs, xo, xc, shape, segment, L, NS, state, is_init, per_row):
    """The CPU path's forward half: (y [B, L, A, 128] with its graph, the leaves it hangs on, the gathered per-row tensors)."""
    N, T, A, _, _ = shape
    B = segment.numel()
    idx, rows = _rows(per_row, segment, L, A)
    h0, flags = _gathered(state, is_init, segment, NS, A, L)
    enc = {f: t.detach().requires_grad_(True) for f, t in net.encoder.items()}
    gru = {f: t.detach().requires_grad_(True) for f, t in net.gru.items()}
    with torch.enable_grad():
        if encoder.stacked_agents(enc) is None:
            feats = PT.encoder(enc, *encoder._gather(xs, xo, xc, idx))                               # [B L, A, 128]
            x = feats.view(B, L, A, H).transpose(1, 2).reshape(B * A, L, H)
            out, _ = rnn.restatement(gru, x, h0, flags.to(x.dtype))
            y = out.view(B, A, L, H).transpose(1, 2)                                                 # [B, L, A, 128]
        else:                                                    # one actor per agent: agent a's rows and sequences on slice a
            gs, go, gc = encoder._gather(xs, xo, xc, idx)
            feats = torch.stack([PT.encoder(P.agent_slice(enc, a), gs[:, a], go[:, a] if go is not None else None, gc[:, a]).reshape(B * L, H)
                                 for a in range(A)], 1)
            x, h4, f4 = feats.view(B, L, A, H), h0.view(B, A, H), flags.view(B, A, L).to(feats.dtype)
            y = torch.stack([rnn.restatement(P.agent_slice(gru, a), x[:, :, a], h4[:, a], f4[:, a])[0] for a in range(A)], 2)
    return y, [*enc.values(), *gru.values()], rows


def _torch_update(net, forward, restate):
    """The CPU path's backward half for both networks: the head's restatement on `forward`'s y (_torch_forward's), autograd from dy back
    through the GRU and the encoder; leaves every parameter's .grad set.  Returns the head's dict."""
    y, leaves, rows = forward
    with torch.no_grad():
        res = restate(net.head, y.detach(), *rows)
    grads = torch.autograd.grad(y, leaves, res["dy"])
    for t, g in zip([*net.encoder.values(), *net.gru.values()], grads):
        t.grad = g
    for f, t in net.head.items():
        t.grad = res["d_" + f].reshape(t.shape).clone()
    return res


def _device_forward_to_y(net, xs, xo, xc, shape, segment, L, NS, state, is_init, ws):
    """encoder -> GRU on the device; returns what the backward half needs."""
    N, T, A, D, K = shape
    dev = xs.device
    B = segment.numel()
    lib = abi.load_library()
    # a bad id is clamped for the encoder and the two gathers (finite features, a stored state): its rows are dead in the head entry, which
    # takes the ids as they are, so dy, hence dx, is zero there and the segment adds nothing to any gradient
    index = _step_index(segment.clamp(0, NS - 1), L)
    stacked = encoder.stacked_agents(net.encoder) is not None
    nb = (lib.hns_encoder_agents_workspace_bytes if stacked else lib.hns_encoder_workspace_bytes)(B * L * A, D, A, K, 1)
    if nb == 0:
        raise ValueError(f"shape outside the kernels' limits: {B * L * A} rows, self_dim {D}, {A} agents, {K} cylinders")
    ews = ws.bytes("encoder", nb, dev)
    feats = ws.floats("features", (B * L, A, H), dev)
    encoder.device_forward(net.encoder, xs, xo, xc, index, shape, workspace=ews, out=feats)
    x4 = feats.view(B, L, A, H).transpose(1, 2)                                                      # [B, A, L, 128]: a view, read in place
    h0, flags = _gathered(state, is_init, segment, NS, A, L)
    view = lambda name: ws.floats(name, (B * L, A, H), dev).view(B, L, A, H).transpose(1, 2)         # noqa: E731
    y, _, hist = rnn.device_forward(net.gru, x4, h0, flags, True, out=view("y"), h_last=ws.floats("h_last", (B * A, H), dev),
                                    h_hist=ws.floats("h_hist", (B * A, L, H), dev))
    return index, ews, x4, h0, flags, y, hist, view


def _rows_struct(y, segment, NS):
    r = abi.HnsRnnRows()
    B, A, L, _ = y.shape
    r.y = y.data_ptr()
    for d in range(3):
        r.y_stride[d] = y.stride(d) if y.shape[d] > 1 else 0
    r.outer, r.inner, r.steps = B, A, L
    r.segment = segment.data_ptr()
    r.num_segments = NS
    return r


def _device_backward(net, bucket, xs, xo, xc, shape, index, ews, x4, h0, flags, hist, dy, view, ws):
    """dy -> the GRU's and the encoder's gradients, written into the bucket's slices."""
    dev = xs.device
    B, A, L, _ = x4.shape
    n_enc = encoder.grad_layout(net.encoder)[1]
    agents, lib = rnn.stacked_agents(net.gru), abi.load_library()
    n_gru = rnn.grad_layout(agents)[1]
    gws = ws.bytes("gru", lib.hns_gru_workspace_bytes(B * A, L, 1) if agents is None else lib.hns_gru_agents_workspace_bytes(B, A, L, 1), dev)
    dxbuf = ws.floats("dx", (B * L, A, H), dev)
    rnn.device_backward(net.gru, x4, h0, flags, hist, dy, None, False, workspace=gws, flat=bucket.flat[n_enc:n_enc + n_gru],
                        dx=dxbuf.view(B, L, A, H).transpose(1, 2))
    encoder.device_backward(net.encoder, xs, xo, xc, index, shape, dxbuf, workspace=ews, flat=bucket.flat[:n_enc])


class _Forward:
    """value_loss_sums_rnn's forward state for value_loss_and_grad_rnn(forward=): opaque.  On the device the tensors lie in the caller's
    RnnWorkspace (y, h_hist, the features) or are the call's own (the gathered h0 / flags, the index); on the CPU it is y with its graph."""

    def __init__(self, key, state):
        self.key, self.state = key, state


def _forward_key(net, xs, segment, L, ws):
    return (id(net.head["head_w"]), xs.data_ptr(), tuple(xs.shape), segment.data_ptr(), segment.numel(), L, id(ws))


# What varies between the entries below, the head: actor (or critic); per_row: (name, tensor, values per agent row) of the update's own
# tensors; keys, row_key: the scalars and the per-row result in the restatement's dict, in the result's order (no keys: the forward-only head
# of value_loss_sums_rnn); restate(head parameters, y, *gathered rows): the CPU statements; launch(lib, head parameters, hns_rnn_rows, the
# per-row tensors, dy, the head's gradient views, the result slots, head workspace, its bytes, stream, (B, L, A)): the C call, returning
# the per-row result; check(device): the caller's refusals that need the prepared tensors; stacked: one actor per agent — the network's
# tensors are the stacked ones and the head entry the _agents form.
_Head = collections.namedtuple("_Head", ["actor", "per_row", "keys", "row_key", "restate", "launch", "check", "stacked"], defaults=(None, False))


def _run(head, network, obs, state, is_init, segment, seq_len, check_index, workspace=None, out=None, bucket=None, global_rows=None, group=None,
         forward=None):
    """The one path behind the three entries, for both networks, the local and the global form, the CPU and the device: prepare, forward to y
    (or go on from `forward`), the head, backward from dy into the bucket, the norm.  Returns (the head's scalars, grad_norm, its per-row
    result) — or, for the forward-only head, (sums, values, the forward state)."""
    word = "actor" if head.actor else "critic"
    net = network_parameters(network, head.actor, head.stacked)
    xs, xo, xc, shape, segment, L, NS = _prepare(word, net, obs, state, is_init, head.per_row, segment, seq_len, check_index and forward is None)
    A, B, glob = shape[2], segment.numel(), global_rows is not None
    if glob or group is not None:
        PT.check_global(word, dict(enumerate(flat_parameters(net))), global_rows, B * L * A, group, bucket)
    if head.check is not None:
        head.check(xs.device)
    if forward is not None and (not isinstance(forward, _Forward) or forward.key != _forward_key(net, xs, segment, L, workspace if xs.is_cuda else None)):
        raise ValueError("forward= must be value_loss_sums_rnn's state of the same critic, observations, segment tensor, seq_len and workspace")
    if not xs.is_cuda:
        fwd = forward.state if forward is not None else _torch_forward(net, xs, xo, xc, shape, segment, L, NS, state, is_init,
                                                                       [(t, w) for _, t, w in head.per_row])
        if not head.keys:
            with torch.no_grad():
                sums, v = head.restate(net.head, fwd[0].detach(), *fwd[2])
            return sums, v.unsqueeze(-1), _Forward(_forward_key(net, xs, segment, L, None), fwd)
        res = _torch_update(net, fwd, head.restate)
        if not glob:
            with torch.no_grad():                                # clip_grad_norm_'s total norm
                norm = torch.nn.utils.clip_grad_norm_(flat_parameters(net), float("inf"))
        else:                                                    # the data-parallel call: the bucket's norm after its all-reduce
            if bucket is not None:
                bucket.adopt()
            norm = PT.finish_global(bucket, group)
            norm = norm.reshape(()) if norm is not None else None
        return [res[k] for k in head.keys], norm, res[head.row_key].unsqueeze(-1)
    dev, lib, n = xs.device, abi.load_library(), len(head.keys)
    ws = workspace if workspace is not None else RnnWorkspace()
    scal = None
    if head.keys:
        if not (glob and bucket is None):
            bucket = _bucket(net, bucket)
        scal = PT.check_out(out, n + 1, dev) if out is not None else torch.empty(n + 1, dtype=torch.float32, device=dev)
    per_row = [t.contiguous() for _, t, _ in head.per_row]
    fwd = forward.state[0] if forward is not None else _device_forward_to_y(net, xs, xo, xc, shape, segment, L, NS, state, is_init, ws)
    index, ews, x4, h0, flags, y, hist, view = fwd
    nbytes = (lib.hns_rnn_actor_head_agents_workspace_bytes if head.stacked else
              lib.hns_rnn_actor_head_workspace_bytes if head.actor else lib.hns_rnn_critic_head_workspace_bytes)(B, A, L)
    call = (lib, net.head, _rows_struct(y, segment, NS), per_row)
    tail = (ws.bytes("head", nbytes, dev), nbytes, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), (B, L, A))
    if not head.keys:
        with torch.cuda.device(dev):
            sums, values = head.launch(*call, None, None, None, *tail)
        return sums, values, _Forward(_forward_key(net, xs, segment, L, ws), (fwd, segment))
    dy = view("dy")
    own = bucket if bucket is not None else PT.GradBucket(flat_parameters(net))        # (global_rows without a bucket: the gradients only)
    with torch.cuda.device(dev):
        rows_out = head.launch(*call, dy, dict(zip(net.head, own.views[len(net.encoder) + len(net.gru):])), scal, *tail)
    _device_backward(net, own, xs, xo, xc, shape, index, ews, x4, h0, flags, hist, dy, view, ws)
    norm = PT.finish_global(bucket, group, scal[n:]) if glob else bucket.norm(scal[n:])
    return scal[:n].unbind(), scal[n] if norm is not None else None, rows_out


def policy_loss_and_grad_rnn(actor, obs_self, obs_others, obs_cylinders, actor_rnn_state, is_init, action, log_probs_old, advantages, segment=None,
                             seq_len=16, clip_param=0.1, entropy_coef=0.001, check_index=True, workspace=None, out=None, bucket=None,
                             global_rows=None, entropy_share=1.0, group=None):
    """update_actor_rnn up to the gradient norm: ActorLoss(policy_loss, entropy, ess, grad_norm: 0-dim tensors; log_probs [B, L, A, 1]) and
    every parameter's .grad (views of ONE flat GradBucket on the device: `bucket` (make_bucket), or one made for the call).

    actor: the recurrent actor's parameters under the reference's names (encoder.*, rnn.*, act_dist.*); obs_*: the rollout's [N, T, A, ...]
    observations; actor_rnn_state [N, T / L, A, 128]: the state going into every segment; is_init [N, T, 1]; action [N, T, A, 4],
    log_probs_old, advantages [N, T, A, 1]; segment: int64 [B] ids into the flattened [N, T / L] (None: all, in order); seq_len: L.
    `check_index` range-checks the ids (one host synchronisation); unchecked, an id outside the rollout contributes nothing on the device (its
    rows are dead in the head entry, the encoder and the GRU run on a clamped copy of it) and raises IndexError from torch's gather on the
    CPU.  `workspace`: an RnnWorkspace kept between calls; `out`: four fp32 device values that receive policy_loss, entropy, ess and
    grad_norm.  Both are ignored on the CPU.

    `global_rows` (None: the call above, untouched): this minibatch is one rank's part of a union of `global_rows` rows
    (hns_rnn_actor_head_grad_global): policy_loss is this rank's SHARE, -4 sum_local / global_rows, and the gradients are the share's — over
    the ranks both add up to the union's.  `entropy_share`: the part of the entropy term's gradient this rank adds (1 / world).  ess stays
    this rank's own.  `bucket` is then the network's GradBucket and grad_norm its norm (None without one); `group`: the bucket is all-reduced
    (SUM) over it first."""
    return _policy_loss_and_grad(False, actor, obs_self, obs_others, obs_cylinders, actor_rnn_state, is_init, action, log_probs_old, advantages, segment,
                                 seq_len, clip_param, entropy_coef, check_index, workspace, out, bucket, global_rows, entropy_share, group)


def policy_loss_and_grad_rnn_per_agent(actor, obs_self, obs_others, obs_cylinders, actor_rnn_state, is_init, action, log_probs_old, advantages,
                                       segment=None, seq_len=16, clip_param=0.1, entropy_coef=0.001, check_index=True, workspace=None, out=None,
                                       bucket=None, global_rows=None, group=None):
    """`policy_loss_and_grad_rnn` with one actor per agent (MAPPOPolicy.update_actor with share_actor: False on a recurrent minibatch,
    mappo.py:281-284): `actor` holds the STACKED tensors ([A, ...] each, the `rnn.*` leaves among them), row (b, t, a) and sequence (b, a) run
    on slice a, and every stacked tensor's .grad is as zero_grad() + backward() leave it (agent a's slice from its own rows).  policy_loss is
    -4 times the mean over ALL B L A rows, entropy the mean over the agents of each agent's (each d log_std takes -entropy_coef / A), ess as
    for the shared actor, grad_norm ONE norm over all 29 stacked tensors.  Arguments, layouts, `workspace`, `out` and `bucket`
    (make_bucket(stacked=True)) as `policy_loss_and_grad_rnn`; `is_init` is env-level and holds for all agents.  This is the local call:
    `global_rows=` / `group=` raise NotImplementedError — the data-parallel form is `policy_loss_and_grad_rnn_per_agent_global`."""
    if global_rows is not None or group is not None:
        raise NotImplementedError("policy_loss_and_grad_rnn_per_agent is the local call: the data-parallel form (global_rows=, group=) is "
                                  "rnn_train.policy_loss_and_grad_rnn_per_agent_global")
    return _policy_loss_and_grad(True, actor, obs_self, obs_others, obs_cylinders, actor_rnn_state, is_init, action, log_probs_old, advantages, segment,
                                 seq_len, clip_param, entropy_coef, check_index, workspace, out, bucket, None, 1.0, None)


def policy_loss_and_grad_rnn_per_agent_global(actor, obs_self, obs_others, obs_cylinders, actor_rnn_state, is_init, action, log_probs_old, advantages,
                                              segment=None, seq_len=16, clip_param=0.1, entropy_coef=0.001, check_index=True, workspace=None, out=None,
                                              bucket=None, global_rows=None, entropy_share=1.0, group=None):
    """`policy_loss_and_grad_rnn_per_agent` as one rank's part of a data-parallel update over a union of `global_rows` rows
    (hns_rnn_actor_head_grad_agents_global), with `policy_loss_and_grad_rnn(global_rows=...)`'s semantics: policy_loss is this
    rank's SHARE, every stacked gradient the share's, each agent's d log_std takes (-entropy_coef entropy_share) / A, entropy is the same on
    every rank, ess stays this rank's own.  `bucket` (make_bucket(stacked=True)): the 29 stacked tensors' GradBucket, grad_norm its norm (None
    without one); `group`: the bucket is all-reduced (SUM) over it first.  With global_rows = the call's own B L A and entropy_share 1 every
    output has the local call's bits."""
    if global_rows is None:
        raise ValueError("policy_loss_and_grad_rnn_per_agent_global needs global_rows= (the local call is policy_loss_and_grad_rnn_per_agent)")
    return _policy_loss_and_grad(True, actor, obs_self, obs_others, obs_cylinders, actor_rnn_state, is_init, action, log_probs_old, advantages, segment,
                                 seq_len, clip_param, entropy_coef, check_index, workspace, out, bucket, global_rows, entropy_share, group)


def _policy_loss_and_grad(stacked, actor, obs_self, obs_others, obs_cylinders, actor_rnn_state, is_init, action, log_probs_old, advantages, segment,
                          seq_len, clip_param, entropy_coef, check_index, workspace, out, bucket, global_rows, entropy_share, group):
    """policy_loss_and_grad_rnn and its _per_agent form: the `_Head` of the shared or the stacked head through `_run`."""
    if not clip_param >= 0:
        raise ValueError("clip_param must be >= 0")
    if not math.isfinite(float(entropy_share)):
        raise ValueError("entropy_share must be finite")

    def restate(p, y, a, lpo, adv):
        return actor_head(p["head_w"], p["head_b"], p["log_std"], y, a, lpo, adv, float(clip_param), float(entropy_coef), global_rows,
                          float(entropy_share))

    def launch(lib, p, rows, per_row, dy, g, scal, hws, nbytes, st, dims):
        log_probs = torch.empty(*dims, 1, dtype=torch.float32, device=hws.device)
        entry, more = (lib.hns_rnn_actor_head_grad_agents if stacked else lib.hns_rnn_actor_head_grad, ()) if global_rows is None else \
            (lib.hns_rnn_actor_head_grad_agents_global if stacked else lib.hns_rnn_actor_head_grad_global, (int(global_rows), float(entropy_share)))
        rc = entry(p["head_w"].data_ptr(), p["head_b"].data_ptr(), p["log_std"].data_ptr(), C.byref(rows), *(t.data_ptr() for t in per_row),
                   float(clip_param), float(entropy_coef), dy.data_ptr(), g["head_w"].data_ptr(), g["head_b"].data_ptr(), g["log_std"].data_ptr(),
                   scal[0:].data_ptr(), scal[1:].data_ptr(), scal[2:].data_ptr(), log_probs.data_ptr(), hws.data_ptr(), nbytes, st, *more)
        abi.check(rc, entry.__name__)
        return log_probs

    head = _Head(True, (("action", action, P.ACTION_DIM), ("log_probs_old", log_probs_old, 1), ("advantages", advantages, 1)),
                 ("policy_loss", "entropy", "ess"), "log_probs", restate, launch, None, stacked)
    scalars, norm, log_probs = _run(head, actor, (obs_self, obs_others, obs_cylinders), actor_rnn_state, is_init, segment, seq_len, check_index,
                                    workspace, out, bucket, global_rows, group)
    return ActorLoss(*scalars, norm, log_probs)


def _critic_checks(loss, clip_param, huber_delta):
    if loss not in critic_train.LOSSES:
        raise ValueError(f"loss must be 'huber' or 'mse', not {loss!r}")
    if not clip_param >= 0 or (loss == "huber" and not huber_delta > 0):
        raise ValueError("clip_param must be >= 0 and huber_delta > 0")


def value_loss_sums_rnn(critic, obs_self, obs_others, obs_cylinders, critic_rnn_state, is_init, b_values, b_returns, segment=None, seq_len=16,
                        clip_param=0.1, loss="huber", huber_delta=10.0, check_index=True, workspace=None):
    """The forward half of a data-parallel value_loss_and_grad_rnn: encoder -> GRU -> hns_rnn_critic_head_sums.  Returns
    CriticSumsRnn(sums, values, forward): the five fp64 values of THIS rank's rows (sum loss(v - ret), sum loss(clipped - ret),
    sum (v - ret)^2, sum ret, sum ret^2), values [B, L, A, 1], and the forward state.  No gradient is touched.  The caller adds the ranks' sums
    (one SUM all-reduce) and passes the result to value_loss_and_grad_rnn(sums=, global_rows=, forward=): with `forward` that call goes on
    from y instead of running the encoder and the GRU again.  The state is valid until the next call that uses `workspace` (segment= must
    be the same tensor in both calls).  Arguments and refusals: value_loss_and_grad_rnn's."""
    _critic_checks(loss, clip_param, huber_delta)

    def restate(p, y, bv, ret):
        return critic_head_sums(p["head_w"], p["head_b"], y, bv, ret, float(clip_param), loss, float(huber_delta))

    def launch(lib, p, rows, per_row, dy, g, scal, hws, nbytes, st, dims):
        sums = torch.empty(5, dtype=torch.float64, device=hws.device)
        values = torch.empty(*dims, 1, dtype=torch.float32, device=hws.device)
        rc = lib.hns_rnn_critic_head_sums(p["head_w"].data_ptr(), p["head_b"].data_ptr(), C.byref(rows), *(t.data_ptr() for t in per_row),
                                          float(clip_param), critic_train.LOSSES[loss], float(huber_delta), sums.data_ptr(), values.data_ptr(),
                                          hws.data_ptr(), nbytes, st)
        abi.check(rc, "hns_rnn_critic_head_sums")
        return sums, values

    head = _Head(False, (("b_values", b_values, 1), ("b_returns", b_returns, 1)), (), None, restate, launch)
    return CriticSumsRnn(*_run(head, critic, (obs_self, obs_others, obs_cylinders), critic_rnn_state, is_init, segment, seq_len, check_index, workspace))


def value_loss_and_grad_rnn(critic, obs_self, obs_others, obs_cylinders, critic_rnn_state, is_init, b_values, b_returns, segment=None, seq_len=16,
                            clip_param=0.1, loss="huber", huber_delta=10.0, check_index=True, workspace=None, out=None, bucket=None, sums=None,
                            global_rows=None, group=None, forward=None):
    """update_critic_rnn up to the gradient norm: CriticLoss(value_loss, explained_var, grad_norm: 0-dim tensors; values [B, L, A, 1]) and
    every parameter's .grad.  critic: the recurrent critic's parameters (base.*, rnn.*, v_out.*); critic_rnn_state [N, T / L, A, 128];
    b_values, b_returns [N, T, A, 1]; the other arguments are policy_loss_and_grad_rnn's (`out`: three values).

    `sums`, `global_rows` (both None: the call above, untouched): this minibatch is one rank's part of a union of `global_rows` rows whose
    five fp64 sums are `sums` (value_loss_sums_rnn's over all ranks, added): hns_rnn_critic_head_grad_global takes the branch, value_loss and
    explained_var from them — the same on every rank — and the gradients are this rank's part, which adds up over the ranks to the union's.
    `values` is None on the device (value_loss_sums_rnn returned them).  `forward`: value_loss_sums_rnn's state of the SAME arguments and
    workspace; without it the encoder and the GRU run again.  `bucket`, `group`: policy_loss_and_grad_rnn's."""
    _critic_checks(loss, clip_param, huber_delta)
    if (sums is None) != (global_rows is None):
        raise ValueError("sums= and global_rows= travel together: the union's five sums and its row count")
    if forward is not None and sums is None:
        raise ValueError("forward= belongs to the data-parallel call: pass sums= and global_rows= as well")

    def check(dev):
        if sums is not None and (not torch.is_tensor(sums) or sums.dtype != torch.float64 or sums.numel() != 5 or sums.device != dev or
                                 not sums.is_contiguous()):
            raise ValueError(f"sums must be five contiguous float64 values on {dev}")

    def restate(p, y, bv, ret):
        return critic_head(p["head_w"], p["head_b"], y, bv, ret, float(clip_param), loss, float(huber_delta), sums, global_rows)

    def launch(lib, p, rows, per_row, dy, g, scal, hws, nbytes, st, dims):
        values = None if sums is not None else torch.empty(*dims, 1, dtype=torch.float32, device=hws.device)
        entry, more = (lib.hns_rnn_critic_head_grad, ()) if sums is None else (lib.hns_rnn_critic_head_grad_global, (sums.data_ptr(), int(global_rows)))
        rc = entry(p["head_w"].data_ptr(), p["head_b"].data_ptr(), C.byref(rows), *(t.data_ptr() for t in per_row), float(clip_param),
                   critic_train.LOSSES[loss], float(huber_delta), dy.data_ptr(), g["head_w"].data_ptr(), g["head_b"].data_ptr(), scal[0:].data_ptr(),
                   scal[1:].data_ptr(), values.data_ptr() if values is not None else None, hws.data_ptr(), nbytes, st, *more)
        abi.check(rc, entry.__name__)
        return values

    head = _Head(False, (("b_values", b_values, 1), ("b_returns", b_returns, 1)), ("value_loss", "explained_var"), "values", restate, launch, check)
    scalars, norm, values = _run(head, critic, (obs_self, obs_others, obs_cylinders), critic_rnn_state, is_init, segment, seq_len, check_index,
                                 workspace, out, bucket, global_rows, group, forward)
    return CriticLoss(*scalars, norm, values)


def update_actor_rnn(actor, obs_self, obs_others, obs_cylinders, actor_rnn_state, is_init, action, log_probs_old, advantages, optimizer, segment=None,
                     cfg=None, seq_len=None, check_index=False, workspace=None, out=None, bucket=None, global_rows=None, entropy_share=1.0, group=None):
    """MAPPOPolicy.update_actor on one recurrent minibatch: loss, backward through the head, the GRU and the encoder, clip_grad_norm_, Adam.
    cfg: the algo cfg (clip_param, entropy_coef, actor.rnn.train_seq_len; the reference's defaults when None; seq_len= overrides).  Returns
    {"policy_loss", "actor_grad_norm", "entropy", "ESS"} as 0-dim tensors.  `optimizer`: a ClippedAdam over network_parameters' tensors
    (make_optimizer).  The segment ids are NOT range-checked by default, as update_actor's index.  `global_rows`, `entropy_share`, `group`,
    `bucket`: policy_loss_and_grad_rnn's data-parallel form — forward, the global head entry, backward, the bucket's all-reduce and norm, the
    step, one collective."""
    if global_rows is not None and bucket is None:
        raise ValueError("update_actor_rnn with global_rows= steps on the bucket's norm: pass bucket=")
    PT.check_optimizer(optimizer, "update_actor_rnn", "rnn_train.make_optimizer")
    get = PT.getter(cfg)
    L = int(seq_len) if seq_len is not None else train_seq_len(cfg)
    res = policy_loss_and_grad_rnn(actor, obs_self, obs_others, obs_cylinders, actor_rnn_state, is_init, action, log_probs_old, advantages, segment, L,
                                   float(get("clip_param", 0.1)), float(get("entropy_coef", 0.001)), check_index, workspace, out, bucket,
                                   **(dict(global_rows=global_rows, entropy_share=entropy_share, group=group) if global_rows is not None or group is not None else {}))
    return {"policy_loss": res.policy_loss, "actor_grad_norm": PT.clipped_step(optimizer, res.grad_norm), "entropy": res.entropy, "ESS": res.ess}


def update_actor_rnn_per_agent(actor, obs_self, obs_others, obs_cylinders, actor_rnn_state, is_init, action, log_probs_old, advantages, optimizer,
                               segment=None, cfg=None, seq_len=None, check_index=False, workspace=None, out=None, bucket=None, global_rows=None, group=None):
    """`update_actor_rnn` with one actor per agent (MAPPOPolicy.update_actor with share_actor: False and actor.rnn):
    `policy_loss_and_grad_rnn_per_agent`, then the clip and the Adam step of `optimizer` (make_optimizer_per_agent) over the 29 stacked
    tensors.  The same info dict.  `global_rows=` / `group=` raise NotImplementedError: the data-parallel form is
    `update_actor_rnn_per_agent_global`."""
    if global_rows is not None or group is not None:
        raise NotImplementedError("update_actor_rnn_per_agent is the local call: the data-parallel form (global_rows=, group=) is "
                                  "rnn_train.update_actor_rnn_per_agent_global")
    PT.check_optimizer(optimizer, "update_actor_rnn_per_agent", "rnn_train.make_optimizer_per_agent")
    get = PT.getter(cfg)
    L = int(seq_len) if seq_len is not None else train_seq_len(cfg)
    res = policy_loss_and_grad_rnn_per_agent(actor, obs_self, obs_others, obs_cylinders, actor_rnn_state, is_init, action, log_probs_old, advantages,
                                             segment, L, float(get("clip_param", 0.1)), float(get("entropy_coef", 0.001)), check_index, workspace, out, bucket)
    return {"policy_loss": res.policy_loss, "actor_grad_norm": PT.clipped_step(optimizer, res.grad_norm), "entropy": res.entropy, "ESS": res.ess}


def update_actor_rnn_per_agent_global(actor, obs_self, obs_others, obs_cylinders, actor_rnn_state, is_init, action, log_probs_old, advantages, optimizer,
                                      segment=None, cfg=None, seq_len=None, check_index=False, workspace=None, out=None, bucket=None, global_rows=None,
                                      entropy_share=1.0, group=None):
    """`update_actor_rnn_per_agent` as one rank's part of a data-parallel update: `policy_loss_and_grad_rnn_per_agent_global`
    — forward, the global per-agent head entry, backward, the bucket's all-reduce and norm — then the clip and the Adam step over the 29
    stacked tensors; one collective.  `global_rows` and `bucket` are required (`group` may be None where the caller summed the buckets)."""
    if global_rows is None or bucket is None:
        raise ValueError("update_actor_rnn_per_agent_global steps on the bucket's norm over the union: pass global_rows= and bucket=")
    PT.check_optimizer(optimizer, "update_actor_rnn_per_agent_global", "rnn_train.make_optimizer_per_agent")
    get = PT.getter(cfg)
    L = int(seq_len) if seq_len is not None else train_seq_len(cfg)
    res = policy_loss_and_grad_rnn_per_agent_global(actor, obs_self, obs_others, obs_cylinders, actor_rnn_state, is_init, action, log_probs_old,
                                                    advantages, segment, L, float(get("clip_param", 0.1)), float(get("entropy_coef", 0.001)), check_index,
                                                    workspace, out, bucket, global_rows, entropy_share, group)
    return {"policy_loss": res.policy_loss, "actor_grad_norm": PT.clipped_step(optimizer, res.grad_norm), "entropy": res.entropy, "ESS": res.ess}


def update_critic_rnn(critic, obs_self, obs_others, obs_cylinders, critic_rnn_state, is_init, b_values, b_returns, optimizer, segment=None, cfg=None,
                      seq_len=None, check_index=False, workspace=None, out=None, bucket=None, sums=None, global_rows=None, group=None):
    """MAPPOPolicy.update_critic on one recurrent minibatch; cfg: clip_param, critic.use_huber_loss, critic.huber_delta,
    actor.rnn.train_seq_len.  Returns {"value_loss", "critic_grad_norm", "explained_var"} as 0-dim tensors.  `global_rows`, `bucket`: one
    rank's part of a data-parallel update over a union of `global_rows` rows.  With `group` the call runs value_loss_sums_rnn, the SUM
    all-reduce of the five values, value_loss_and_grad_rnn(sums=, forward=, group=) — ONE encoder and GRU pass — and the step; `sums` given
    instead: the caller added the ranks' sums itself."""
    if global_rows is not None and bucket is None:
        raise ValueError("update_critic_rnn with global_rows= steps on the bucket's norm: pass bucket=")
    if global_rows is not None and sums is None and group is None:
        raise ValueError("update_critic_rnn with global_rows= needs the union's sums= or the group= to add them over")
    PT.check_optimizer(optimizer, "update_critic_rnn", "rnn_train.make_optimizer")
    get, sget = PT.getter(cfg), PT.getter(PT.getter(cfg)("critic", None))
    L = int(seq_len) if seq_len is not None else train_seq_len(cfg)
    hyper = (float(get("clip_param", 0.1)), "huber" if sget("use_huber_loss", True) else "mse", float(sget("huber_delta", 10.0)))
    kw = {}
    if global_rows is not None or group is not None or sums is not None:
        kw = dict(sums=sums, global_rows=global_rows, group=group)
        if global_rows is not None and sums is None:
            from . import sharding
            if segment is not None:
                segment = segment.contiguous()                   # (the forward state is tied to the tensor both calls see)
            half = value_loss_sums_rnn(critic, obs_self, obs_others, obs_cylinders, critic_rnn_state, is_init, b_values, b_returns, segment, L, *hyper,
                                       check_index, workspace)
            kw["sums"] = sharding.all_reduce_sum(half.sums, group)
            if segment is not None:
                kw["forward"] = half.forward
    res = value_loss_and_grad_rnn(critic, obs_self, obs_others, obs_cylinders, critic_rnn_state, is_init, b_values, b_returns, segment, L, *hyper,
                                  check_index, workspace, out, bucket, **kw)
    return {"value_loss": res.value_loss, "critic_grad_norm": PT.clipped_step(optimizer, res.grad_norm), "explained_var": res.explained_var}


def train_seq_len(cfg):
    """cfg.actor.rnn.train_seq_len (cfg/algo/mappo.yaml's key), default 16."""
    sub = PT.getter(PT.getter(PT.getter(cfg)("actor", None))("rnn", None))
    return int(sub("train_seq_len", 16) or 16)
