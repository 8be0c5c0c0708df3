"""The MAPPO policy's forward pass on the device: MAPPOPolicy.__call__ and value_op (learning/mappo.py:221-250) for HideAndSeek.

The reference's network for this task, at cfg/algo/mappo.yaml's defaults (share_actor: True, critic_input: obs, no rnn, tanh: false), is a
PartialAttentionEncoder per network (modules/networks.py:250-313: SplitEmbedding over state_self / state_others / cylinders, LayerNorm,
single-query attention, a GELU feed-forward and two more LayerNorms; embed_dim 128), a DiagGaussian head for the actor (fc_mean 128 -> 4,
scale = exp(log_std)) and v_out 128 -> 1 for the critic.  `DevicePolicy` runs both networks for every (env, agent) row in ONE call of
`hns_policy_forward`: loc, an action (a sample, or the mode with deterministic=True), its log_prob and the critic's value.  `act` runs the
actor alone for the mode (`hns_policy_act`: evaluation).  The noise is the
caller's eps, or Philox4x32-10 drawn in the kernel from (seed, device call counter, row) — a captured graph draws fresh noise on every replay.

Parameters come from the reference's live objects (`actor_params`, a TensorDictParams of the shared actor, and the critic module) or from a
checkpoint written by scripts/train.py (`MAPPOPolicy.state_dict()`: "actor_params", "critic").  Names are accepted with or without
TensorDictModule's `module.` prefix.  The packed operand image is rebuilt on the device when a parameter's data_ptr or version counter moves,
so the next call follows an optimiser step (as env.HideAndSeek._tp_sync_weights does for the predictor).

CPU tensors run a torch restatement of the reference's statements (tests, gloo runs — not the hot path).  DESIGN.md §7.3.

`RecurrentDevicePolicy` is the `actor.rnn` / `critic.rnn` configuration (a GRU behind each encoder, modules/rnn.py): encoder -> one GRU step ->
head for both networks in ONE call of `hns_policy_forward_rnn`, the two states carried on the device; its `act_step` runs
the actor's half alone with the actor's state (`hns_policy_act_rnn`: evaluation).  `DevicePolicy` keeps refusing that
configuration.

`PerAgentDevicePolicy` is the `share_actor: False` configuration (one actor per agent: the stacked `actor_params`, every tensor [A, ...]; the
critic shared) on `hns_policy_forward_agents` / `hns_policy_act_agents`: a tile is 32 envs of ONE agent and reads that agent's weight image,
and agent a's rows are bit for bit `DevicePolicy`'s with slice a as the shared actor.  `DevicePolicy` keeps refusing
stacked parameters.

`PerAgentRecurrentDevicePolicy` is both at once — the configuration the reference's recurrent update is written for (mappo.py:281-284 vmaps
over dim 0 of the stacked `actor_params`): one actor AND one actor GRU per agent, the critic and its GRU shared, on
`hns_policy_forward_rnn_agents` / `hns_policy_act_rnn_agents` in §7.16's tile, the state rows where they were ([E, A, 128]); row (e, a) is bit
for bit `RecurrentDevicePolicy`'s with agent a's slices.  Collection and evaluation only: its update is an open item.

`CentralCriticDevicePolicy` is the `critic_input: state` configuration (the centralised critic: ONE encoder row per env over the state spec
— the A rows of state_drones through one embedding, then the cylinders — and v_out = Linear(128, A)) beside the shared non-recurrent actor on
`hns_policy_central_forward`: actor tiles of 32 (env, agent) rows and critic tiles of 32 envs in one launch, the actor's outputs bit for bit
`DevicePolicy`'s.  The four classes above keep refusing that configuration.

`PerAgentCentralCriticDevicePolicy` is share_actor: False AND critic_input: state — heterogeneous actors under one critic over the joint state,
the canonical centralised-training / decentralised-execution setup — on `hns_policy_central_forward_agents`: per agent a range of actor tiles
of 32 envs, then one range of critic tiles of 32 envs, in one launch; action, log_prob and loc are bit for bit `PerAgentDevicePolicy`'s and
value bit for bit `CentralCriticDevicePolicy`'s.  The five classes above keep their refusals.

Layout of this file, as the device side's (one tile body, three flags): the configuration checks and the parsers (`parse_parameters` and
`split_rnn`, each with a `stacked` switch); ONE CPU restatement (`_restatement`: a GRU step or not, a stacked actor or not, the actor's half
alone or not; `torch_forward` and `torch_forward_rnn` are its public forms); the random builders; `ENTRIES`, the eight C entries keyed
(agents, rnn, act) as kPolKernels of hns_policy.hip; and `DevicePolicy`, which holds the one host path of all eight (`_pass`) with one
`_validate`, `refresh` and `scale`, switched by its class attributes `per_agent` and `recurrent`.  The three subclasses set those
attributes, parse their parameters and adapt the arguments of `forward`, `act` and `act_step`."""
import collections
import ctypes as C
import math

import torch
import torch.nn.functional as F

from . import abi

EMBED_DIM = 128
ACTION_DIM = 4
KEYS = ("state_self", "state_others", "cylinders")          # spec order of the observation CompositeSpec (env._set_specs)

# reference parameter names (after `module.`) of one PartialAttentionEncoder -> hns_policy_net fields
_ENCODER = {
    "split_embed.embed.state_self.weight": "embed_self_w", "split_embed.embed.state_self.bias": "embed_self_b",
    "split_embed.embed.state_others.weight": "embed_others_w", "split_embed.embed.state_others.bias": "embed_others_b",
    "split_embed.embed.cylinders.weight": "embed_cyl_w", "split_embed.embed.cylinders.bias": "embed_cyl_b",
    "split_embed.layer_norm.weight": "ln_w", "split_embed.layer_norm.bias": "ln_b",
    "attn.in_proj_weight": "in_proj_w", "attn.in_proj_bias": "in_proj_b",
    "attn.out_proj.weight": "out_proj_w", "attn.out_proj.bias": "out_proj_b",
    "linear1.weight": "linear1_w", "linear1.bias": "linear1_b", "linear2.weight": "linear2_w", "linear2.bias": "linear2_b",
    "norm1.weight": "norm1_w", "norm1.bias": "norm1_b", "norm2.weight": "norm2_w", "norm2.bias": "norm2_b",
}
ACTOR_NAMES = {**{"encoder." + k: v for k, v in _ENCODER.items()},
               "act_dist.fc_mean.weight": "head_w", "act_dist.fc_mean.bias": "head_b", "act_dist.log_std": "log_std"}
CRITIC_NAMES = {**{"base." + k: v for k, v in _ENCODER.items()}, "v_out.weight": "head_w", "v_out.bias": "head_b"}

# the centralised critic (critic_input: state; make_critic(centralized=True), mappo.py:553-566): the encoder over the STATE spec — state_drones
# (every drone's row through ONE embedding, here under hns_policy_net's embed_self_*) and cylinders, no state_others — and v_out = Linear(128, A)
CENTRAL_CRITIC_NAMES = {**{"base." + k.replace("state_self", "state_drones"): v for k, v in _ENCODER.items() if "state_others" not in k},
                        "v_out.weight": "head_w", "v_out.bias": "head_b"}

PolicyOutput = collections.namedtuple("PolicyOutput", ["action", "log_prob", "value", "loc"])
RecurrentPolicyOutput = collections.namedtuple("RecurrentPolicyOutput", ["action", "log_prob", "value", "loc", "actor_state", "critic_state"])


class PolicyConfigError(ValueError):
    """The network or configuration is one this forward pass does not implement."""


def getter(cfg):
    """get(key, default) of a cfg section, whether it is a mapping, an attribute object or None (every default)."""
    if cfg is None:
        return lambda k, d=None: d
    return cfg.get if hasattr(cfg, "get") else (lambda k, d=None: getattr(cfg, k, d))


def cfg_without(cfg, *dotted_keys):
    """The cfg (a mapping, an attribute object or None, which stays None) as a dict without `dotted_keys` — "share_actor"; "actor.rnn": the
    key rnn of the section actor — and with every other key kept: what a check written for another configuration is asked about."""
    if cfg is None:
        return None
    get = getter(cfg)
    out = {k: get(k) for k in (cfg.keys() if hasattr(cfg, "keys") else [k for k in vars(cfg) if not k.startswith("_")])}
    for dotted in dotted_keys:
        key, _, rest = dotted.partition(".")
        if not rest:
            out.pop(key, None)
        elif out.get(key) is not None:
            out[key] = cfg_without(out[key], rest)
    return out


def check_config(cfg):
    """Refuse the algo configurations the device forward pass does not cover (cfg: the algo cfg mapping, or None)."""
    if cfg is None:
        return
    get = getter(cfg)
    if not get("share_actor", True):
        raise PolicyConfigError("share_actor: False (one actor per agent) is not supported; only the shared actor is")
    if get("critic_input", "obs") != "obs":
        raise PolicyConfigError(f"critic_input: {get('critic_input')} (the centralised critic) is not supported; only critic_input: obs is")
    for part in ("actor", "critic"):
        sget = getter(get(part, None))
        if sget("rnn", None):
            raise PolicyConfigError(f"{part}.rnn is not supported")
        if part == "actor" and sget("tanh", False):
            raise PolicyConfigError("actor.tanh: true (TanhNormal) is not supported; only the DiagGaussian actor is")


def _flatten(obj, prefix=""):
    """name -> tensor from an nn.Module, a TensorDict-like (flatten_keys / items) or a (nested) mapping; `module.` prefixes dropped."""
    if hasattr(obj, "named_parameters") and not hasattr(obj, "flatten_keys"):
        items = list(obj.named_parameters())
        if not items:
            items = list(obj.state_dict(keep_vars=True).items())
    elif hasattr(obj, "flatten_keys"):
        flat = obj.flatten_keys(".")
        items = list(flat.items())
    elif hasattr(obj, "items"):
        out = {}
        for k, v in obj.items():
            k = ".".join(k) if isinstance(k, tuple) else str(k)
            if torch.is_tensor(v):
                out[prefix + k] = v
            else:
                out.update(_flatten(v, prefix + k + "."))
        return out
    else:
        raise TypeError(f"cannot read parameters from {type(obj).__name__}")
    out = {}
    for k, v in items:
        k = ".".join(k) if isinstance(k, tuple) else str(k)
        out[prefix + k] = v
    return out


def _strip(name):
    while name.startswith("module."):
        name = name[len("module."):]
    return name


def _stacked_agents(tensors, what, kind, plural, show):
    """A, the one leading size of stacked tensors, in [1, HNS_MAX_AGENTS]; `kind`, `plural` and `show` word the two refusals."""
    sizes = {int(v.shape[0]) if v.dim() else None for v in tensors}
    if len(sizes) != 1 or None in sizes:
        raise PolicyConfigError(f"{what}: every stacked {kind}tensor needs the same leading agent dimension, not {sorted(show(s) for s in sizes)}")
    A = sizes.pop()
    if not 1 <= A <= abi.HNS_MAX_AGENTS:
        raise PolicyConfigError(f"{what}: {A} stacked {plural} outside [1, {abi.HNS_MAX_AGENTS}]")
    return A


def parse_parameters(params, names, what, stacked=False, central=False):
    """The hns_policy_net fields of one network from reference parameter names; raises PolicyConfigError on anything it does not implement.
    central (the centralised critic, names = CENTRAL_CRITIC_NAMES): the head is Linear(128, A) with A in [1, 7] and a
    state_others or state_self embedding is refused by name.
    stacked (share_actor: False, mappo.py:148-152): (the fields of the STACKED network, every tensor [A, ...]; A) — each
    agent's slice is held to the checks below; tensors that are not stacked, or whose leading sizes disagree, raise PolicyConfigError."""
    flat = {_strip(k): v for k, v in _flatten(params).items()}
    if stacked:
        w = next((v for k, v in flat.items() if names.get(k) == "in_proj_w"), None)
        if w is not None and w.dim() == 2:
            raise PolicyConfigError(f"{what}: the parameters have no leading agent dimension (a shared actor is DevicePolicy's)")
        A = _stacked_agents(flat.values(), what, "", "actors", str)
        first = parse_parameters({k: v[0] for k, v in flat.items()}, names, what)         # names, shapes, dtypes: every slice has slice 0's
        if ("embed_others_w" in first) != (A > 1):
            raise PolicyConfigError(f"{what}: {A} stacked actors {'need' if A > 1 else 'have no'} state_others embedding")
        return {names[k]: v for k, v in flat.items()}, A
    out, unknown = {}, []
    for k, v in flat.items():
        if k in names:
            out[names[k]] = v
        else:
            unknown.append(k)
    if central and any(".state_others." in k or ".state_self." in k for k in unknown):
        raise PolicyConfigError(f"{what}: the centralised critic embeds state_drones and cylinders, not "
                                f"{sorted(k for k in unknown if '.state_others.' in k or '.state_self.' in k)[:4]} (a critic on the observation is "
                                "DevicePolicy's)")
    if any(".rnn." in "." + k or k.startswith("rnn.") for k in unknown):
        raise PolicyConfigError(f"{what}: an rnn is not supported ({[k for k in unknown if 'rnn' in k][:3]})")
    if unknown:
        raise PolicyConfigError(f"{what}: parameters this network does not have: {sorted(unknown)[:6]} (centralised critic, tanh actor or another "
                                "encoder?)")
    required = set(names.values()) - {"embed_others_w", "embed_others_b"}
    missing = sorted(required - set(out))
    if missing:
        raise PolicyConfigError(f"{what}: missing parameters {missing}")
    E = EMBED_DIM
    w = out["in_proj_w"]
    if w.dim() != 2:
        raise PolicyConfigError(f"{what}: parameters with a leading agent dimension (share_actor: False) are not supported")
    if tuple(w.shape) != (3 * E, E) or tuple(out["linear1_w"].shape) != (E, E) or tuple(out["linear2_w"].shape) != (E, E):
        raise PolicyConfigError(f"{what}: embed_dim and dim_feedforward must be 128 (in_proj_weight {tuple(w.shape)}, linear1 "
                                f"{tuple(out['linear1_w'].shape)})")
    heads = ACTION_DIM if "log_std" in names.values() else 1
    if central:
        heads = int(out["head_w"].shape[0]) if out["head_w"].dim() == 2 else 0
        if not 1 <= heads <= abi.HNS_MAX_AGENTS:
            raise PolicyConfigError(f"{what}: v_out must be Linear(128, A) with A in [1, {abi.HNS_MAX_AGENTS}], not {tuple(out['head_w'].shape)}")
    if tuple(out["head_w"].shape) != (heads, E) or tuple(out["head_b"].shape) != (heads,):
        raise PolicyConfigError(f"{what}: the head must be Linear(128, {heads}), not {tuple(out['head_w'].shape)}")
    if "log_std" in out and tuple(out["log_std"].shape) != (ACTION_DIM,):
        raise PolicyConfigError(f"{what}: log_std must have {ACTION_DIM} values")
    if tuple(out["embed_cyl_w"].shape) != (E, 5):
        raise PolicyConfigError(f"{what}: the cylinders embedding must be Linear(5, 128)")
    if ("embed_others_w" in out) and tuple(out["embed_others_w"].shape) != (E, 3):
        raise PolicyConfigError(f"{what}: the state_others embedding must be Linear(3, 128)")
    sw = out["embed_self_w"]
    if sw.dim() != 2 or sw.shape[0] != E or not 1 <= sw.shape[1] <= abi.HNS_POLICY_MAX_SELF_DIM:
        raise PolicyConfigError(f"{what}: the {'state_drones' if central else 'state_self'} embedding must be Linear(D, 128) with D in "
                                f"[1, {abi.HNS_POLICY_MAX_SELF_DIM}]")
    for k, v in out.items():
        if v.dtype != torch.float32:
            raise TypeError(f"{what}: parameter {k} must be float32, not {v.dtype}")
    return out


def parse_parameters_per_agent(params, what="actor"):
    """`parse_parameters` of the stacked actor: (its fields, every tensor [A, ...]; A)."""
    return parse_parameters(params, ACTOR_NAMES, what, stacked=True)


def parse_parameters_central(critic, what="critic"):
    """`parse_parameters` of the centralised critic's 20 tensors: (its fields — embed_self_* hold the state_drones embedding —, A = v_out's rows)."""
    p = parse_parameters(critic, CENTRAL_CRITIC_NAMES, what, central=True)
    return p, int(p["head_w"].shape[0])


def agent_slice(actor_p, a):
    """Agent a's network out of the stacked one: views, a `parse_parameters` dict of its own."""
    return {k: v[a] for k, v in actor_p.items()}


def is_stacked(params, name="encoder.attn.in_proj_weight"):
    """Whether `params` (any source `parse_parameters` reads) holds the stacked actor of share_actor: False: its in_proj_weight is [A, 384, 128]."""
    if params is None:
        return False
    w = {_strip(k): v for k, v in _flatten(params).items()}.get(name)
    return w is not None and w.dim() == 3


def split_rnn(params, what, stacked=False):
    """(the network's parameters without its GRU, the GRU's six tensors by hns_gru_net field) from reference names: the GRU sits under
    `rnn.` (rnn.cell.weight_ih, ..., rnn.layer_norm.bias).  stacked: (the stacked parameters without the GRUs, the GRUs' six
    STACKED tensors — every one [A, ...], contiguous —, A); each agent's slice is held to `gru_parameters`' checks, and rnn tensors that are
    not stacked, or whose leading sizes disagree, raise PolicyConfigError."""
    from . import rnn as _rnn
    flat = {_strip(k): v for k, v in _flatten(params).items()}
    rest = {k: v for k, v in flat.items() if not k.startswith("rnn.")}
    found = {k[len("rnn."):]: v for k, v in flat.items() if k.startswith("rnn.")}
    unknown = sorted(k for k in found if k not in _rnn.NAMES)
    if unknown:
        raise PolicyConfigError(f"{what}: rnn parameters the GRU block does not have: {unknown[:6]}")
    missing = sorted(k for k in _rnn.NAMES if k not in found)
    if missing:
        raise PolicyConfigError(f"{what}: no GRU under 'rnn.' (missing {['rnn.' + k for k in missing]}); a network without an rnn is "
                                "DevicePolicy's")
    if stacked:
        if any(v.dim() != (3 if k.endswith("weight_ih") or k.endswith("weight_hh") else 2) for k, v in found.items()):
            raise PolicyConfigError(f"{what}: the rnn tensors have no leading agent dimension (a shared recurrent actor is RecurrentDevicePolicy's)")
        A = _stacked_agents(found.values(), what, "rnn ", "GRUs", int)
    gru = {_rnn.NAMES[k]: (v if v.is_contiguous() else v.detach().contiguous()) for k, v in found.items()}

    def checked(p, whose):
        try:
            return _rnn.gru_parameters(p)
        except ValueError as e:
            raise PolicyConfigError(f"{what}: {whose} must be GRUCell(128, 128) + LayerNorm(128): {e}") from None

    if not stacked:
        return rest, checked(gru, "the rnn")
    for a in range(A):
        checked(agent_slice(gru, a), f"agent {a}'s rnn")
    return rest, {f: gru[f] for f in _rnn.FIELDS}, A


def check_config_per_agent(cfg):
    """`check_config` for one actor per agent: everything it refuses but share_actor: False; share_actor: True is refused instead."""
    if getter(cfg)("share_actor", False):
        raise PolicyConfigError("share_actor: True with one actor per agent; the shared actor is DevicePolicy's")
    check_config(cfg_without(cfg, "share_actor"))


def check_config_central(cfg):
    """`check_config` for the centralised critic: everything it refuses but critic_input: state; critic_input: obs is refused instead (a cfg
    that does not say, like no cfg, is taken at the class's word — as check_config_per_agent takes share_actor)."""
    if getter(cfg)("critic_input", "state") != "state":
        raise PolicyConfigError(f"critic_input: {getter(cfg)('critic_input')} with the centralised critic; the critic on the observation is "
                                "DevicePolicy's")
    check_config(cfg_without(cfg, "critic_input"))


def check_config_per_agent_central(cfg):
    """`check_config` for one actor per agent beside the centralised critic: both switches are accepted (a cfg that does not say is taken at
    the class's word), share_actor: True and critic_input: obs are refused as the two checks above refuse them, and so is everything else
    `check_config` refuses."""
    if getter(cfg)("share_actor", False):
        raise PolicyConfigError("share_actor: True with one actor per agent; the shared actor beside the centralised critic is "
                                "CentralCriticDevicePolicy's")
    if getter(cfg)("critic_input", "state") != "state":
        raise PolicyConfigError(f"critic_input: {getter(cfg)('critic_input')} with the centralised critic; per-agent actors beside the critic on "
                                "the observation are PerAgentDevicePolicy's")
    check_config(cfg_without(cfg, "share_actor", "critic_input"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# torch restatement (CPU path): the reference's statements, modules/networks.py:125-163, :250-313, distributions.py:66-82, mappo.py:591-660
def _encoder(p, xs, xo, xc):
    toks = [F.linear(xs, p["embed_self_w"], p["embed_self_b"])]
    if xo is not None:
        toks.append(F.linear(xo, p["embed_others_w"], p["embed_others_b"]))
    toks.append(F.linear(xc, p["embed_cyl_w"], p["embed_cyl_b"]))
    x = F.layer_norm(torch.cat(toks, dim=-2), (EMBED_DIM,), p["ln_w"], p["ln_b"])
    lead = x.shape[:-2]
    x = x.reshape(-1, x.shape[-2], EMBED_DIM)
    q = x[:, [0]]
    attn = F.multi_head_attention_forward(q.transpose(0, 1), x.transpose(0, 1), x.transpose(0, 1), EMBED_DIM, 1, p["in_proj_w"], p["in_proj_b"],
                                          None, None, False, 0.0, p["out_proj_w"], p["out_proj_b"], training=False, need_weights=False)[0]
    x = F.layer_norm(q + attn.transpose(0, 1), (EMBED_DIM,), p["norm1_w"], p["norm1_b"])
    x = F.layer_norm(x + F.linear(F.gelu(F.linear(x, p["linear1_w"], p["linear1_b"])), p["linear2_w"], p["linear2_b"]), (EMBED_DIM,),
                     p["norm2_w"], p["norm2_b"])
    return x.mean(-2).reshape(*lead, EMBED_DIM)


def _heads(actor, y_actor, eps, deterministic):
    """(action, log_prob, loc) of the DiagGaussian head on the actor's features; eps: the noise of a sampled action."""
    loc = F.linear(y_actor, actor["head_w"], actor["head_b"])
    scale = torch.broadcast_to(torch.exp(actor["log_std"]), loc.shape)
    action = loc if deterministic else loc + scale * eps
    log_prob = torch.distributions.Normal(loc, scale).log_prob(action).sum(-1, keepdim=True)
    return action, log_prob, loc


def _rnn_step(p, rnn_p, xs, xo, xc, state, is_init):
    """One network's (LayerNorm(h' + f) [E, A, 128], h' [E, A, 128]): `_encoder`, then rnn.restatement over one step (Actor.forward /
    Critic.forward with self.rnn set, mappo.py:603-660)."""
    from . import rnn as _rnn
    f = _encoder(p, xs, xo, xc)
    E, A, _ = f.shape
    h0 = state.reshape(E * A, EMBED_DIM).to(f.dtype) if state is not None else f.new_zeros(E * A, EMBED_DIM)
    if is_init is None:
        m = f.new_zeros(E * A, 1)
    else:
        m = (is_init.reshape(E, 1) != 0).expand(E, A).reshape(E * A, 1).to(f.dtype)          # the env's flag for all of its agents
    out, h = _rnn.restatement(rnn_p, f.reshape(E * A, 1, EMBED_DIM), h0, m)
    return out.reshape(E, A, EMBED_DIM), h.reshape(E, A, EMBED_DIM)


def _restatement(actor, critic, xs, xo, xc, actor_rnn=None, critic_rnn=None, actor_state=None, critic_state=None, is_init=None, eps=None,
                 deterministic=False, value_only=False, generator=None, stacked=False, actor_only=False):
    """The CPU restatement of all eight entries, any dtype: the critic's features -> value and the actor's features -> head, as (action,
    log_prob, value, loc, actor_state, critic_state).  Three switches: a GRU step behind each encoder (actor_rnn / critic_rnn given; without,
    the states stay None); a STACKED actor (and actor GRU) — a loop over the agents' slices, each run on the WHOLE observation and state and
    keeping its own agent's rows, so agent a's rows are exactly the shared pass's with slice a as the actor (a CPU matrix product's bits
    depend on its shape; this path serves tests, not speed); actor_only — the act entries: the actor's features and F.linear with the head,
    the same statements on the same operands as a deterministic pass, returned as the action, with the actor's state and nothing else.
    A sampled pass without eps draws [E, A, 4] from `generator` once; value_only returns before the actor is touched."""
    def features(p, rnn_p, state):
        return _rnn_step(p, rnn_p, xs, xo, xc, state, is_init) if rnn_p is not None else (_encoder(p, xs, xo, xc), None)

    value = hc = None
    if not actor_only:
        yc, hc = features(critic, critic_rnn, critic_state)
        value = F.linear(yc, critic["head_w"], critic["head_b"])
        if value_only:
            return None, None, value, None, None, hc
        if eps is None and not deterministic:
            eps = torch.randn((*xs.shape[:-2], ACTION_DIM), dtype=xs.dtype, device=xs.device, generator=generator)

    def half(p, rnn_p):
        """One actor's (loc,) or (action, log_prob, loc), then its state if it has a GRU."""
        y, h = features(p, rnn_p, actor_state)
        outs = [F.linear(y, p["head_w"], p["head_b"])] if actor_only else [*_heads(p, y, eps, deterministic)]
        return outs + [h] if rnn_p is not None else outs

    if stacked:
        rows = [[t[:, a:a + 1] for t in half(agent_slice(actor, a), agent_slice(actor_rnn, a) if actor_rnn is not None else None)]
                for a in range(xs.shape[1])]
        outs = [torch.cat(t, dim=1) for t in zip(*rows)]
    else:
        outs = half(actor, actor_rnn)
    ha = outs.pop() if actor_rnn is not None else None
    if actor_only:
        return outs[0], None, None, None, ha, None
    action, log_prob, loc = outs
    return action, log_prob, value, loc, ha, hc


def torch_forward(actor, critic, xs, xo, xc, eps=None, deterministic=False, value_only=False, generator=None):
    """The CPU path: (action, log_prob, value, loc) from parameter dicts in hns_policy_net field names; xs [E, A, 1, D]."""
    return PolicyOutput(*_restatement(actor, critic, xs, xo, xc, eps=eps, deterministic=deterministic, value_only=value_only,
                                      generator=generator)[:4])


def torch_forward_rnn(actor, critic, actor_rnn, critic_rnn, xs, xo, xc, actor_state=None, critic_state=None, is_init=None, eps=None,
                      deterministic=False, value_only=False, generator=None):
    """The CPU restatement of hns_policy_forward_rnn, any dtype: parameter dicts in hns_policy_net / hns_gru_net field names, xs [E, A, 1, D],
    states [E, A, 128] or None (zeros), is_init [E] (or [E, 1]) or None -> RecurrentPolicyOutput."""
    return RecurrentPolicyOutput(*_restatement(actor, critic, xs, xo, xc, actor_rnn, critic_rnn, actor_state, critic_state, is_init, eps,
                                               deterministic, value_only, generator))


def torch_forward_central(actor, critic, xs, xo, xc, state_drones, state_cylinders, eps=None, deterministic=False, value_only=False, generator=None,
                          stacked=False):
    """The CPU restatement of hns_policy_central_forward, any dtype: the shared actor as `torch_forward` runs it (xs [E, A, 1, D]) and the
    centralised critic in the reference's statements (Critic.forward with centralized=True, mappo.py:644-660): the encoder over the state —
    state_drones [E, A, D] and state_cylinders [E, K, 5] are SplitEmbedding's two keys, token 0 (drone 0) the query — and v_out, unflattened
    to value [E, A, 1].  stacked (hns_policy_central_forward_agents): `actor` is the stacked actor and runs as
    `_restatement(stacked=True)` runs it — each agent's slice on the whole observation, keeping its own agent's rows."""
    value = F.linear(_encoder(critic, state_drones, None, state_cylinders), critic["head_w"], critic["head_b"]).unsqueeze(-1)
    if value_only:
        return PolicyOutput(None, None, value, None)
    if eps is None and not deterministic:
        eps = torch.randn((*xs.shape[:-2], ACTION_DIM), dtype=xs.dtype, device=xs.device, generator=generator)
    if stacked:
        slices = [agent_slice(actor, a) for a in range(xs.shape[1])]
        rows = [[t[:, a:a + 1] for t in _heads(p, _encoder(p, xs, xo, xc), eps, deterministic)] for a, p in enumerate(slices)]
        action, log_prob, loc = (torch.cat(t, dim=1) for t in zip(*rows))
    else:
        action, log_prob, loc = _heads(actor, _encoder(actor, xs, xo, xc), eps, deterministic)
    return PolicyOutput(action, log_prob, value, loc)


def _td_get(td, key):
    try:
        return td.get(key, None) if hasattr(td, "get") else td[key]
    except KeyError:
        return None


# ---------------------------------------------------------------------------------------------------------------------------------------
# randomly initialised networks in the reference's names (tests, tools, examples)

def random_rnn_parameters(seed=0):
    """A randomly initialised GRU block under the reference's names with the `rnn.` prefix (orthogonal weights, nn.GRUCell's uniform biases,
    LayerNorm at 1 / 0): merge it into one network's dict of `random_parameters`."""
    g = torch.Generator().manual_seed(seed)
    E = EMBED_DIM
    p = {}
    for n in ("weight_ih", "weight_hh"):
        p[f"rnn.cell.{n}"] = torch.cat([torch.linalg.qr(torch.randn(E, E, generator=g))[0] for _ in range(3)]).contiguous()
    bound = 1.0 / math.sqrt(E)
    for n in ("bias_ih", "bias_hh"):
        p[f"rnn.cell.{n}"] = (torch.rand(3 * E, generator=g) * 2 - 1) * bound
    p["rnn.layer_norm.weight"], p["rnn.layer_norm.bias"] = torch.ones(E), torch.zeros(E)
    return p


def random_parameters(self_dim, num_agents, seed=0):
    """A randomly initialised network of the reference's architecture (PyTorch's default initialisers; DiagGaussian's xavier gain 0.01,
    zero bias, log_std 0; v_out orthogonal): (actor, critic) parameter dicts in the reference's names, CPU fp32."""
    g = torch.Generator().manual_seed(seed)
    E = EMBED_DIM

    def lin(o, i):
        bound = 1.0 / math.sqrt(i)
        return (torch.rand(o, i, generator=g) * 2 - 1) * bound, (torch.rand(o, generator=g) * 2 - 1) * bound

    def encoder(prefix):
        p = {}
        keys = [("state_self", self_dim), ("state_others", 3), ("cylinders", 5)] if num_agents > 1 else [("state_self", self_dim), ("cylinders", 5)]
        for k, i in keys:
            p[f"{prefix}split_embed.embed.{k}.weight"], p[f"{prefix}split_embed.embed.{k}.bias"] = lin(E, i)
        for n in ("split_embed.layer_norm", "norm1", "norm2"):
            p[f"{prefix}{n}.weight"], p[f"{prefix}{n}.bias"] = torch.ones(E), torch.zeros(E)
        bound = math.sqrt(6.0 / (E + E))
        p[f"{prefix}attn.in_proj_weight"] = (torch.rand(3 * E, E, generator=g) * 2 - 1) * bound
        p[f"{prefix}attn.in_proj_bias"] = torch.zeros(3 * E)
        p[f"{prefix}attn.out_proj.weight"], _ = lin(E, E)
        p[f"{prefix}attn.out_proj.bias"] = torch.zeros(E)
        p[f"{prefix}linear1.weight"], p[f"{prefix}linear1.bias"] = lin(E, E)
        p[f"{prefix}linear2.weight"], p[f"{prefix}linear2.bias"] = lin(E, E)
        return p

    actor = encoder("encoder.")
    bound = 0.01 * math.sqrt(6.0 / (E + ACTION_DIM))
    actor["act_dist.fc_mean.weight"] = (torch.rand(ACTION_DIM, E, generator=g) * 2 - 1) * bound
    actor["act_dist.fc_mean.bias"] = torch.zeros(ACTION_DIM)
    actor["act_dist.log_std"] = torch.zeros(ACTION_DIM)
    critic = encoder("base.")
    q, _ = torch.linalg.qr(torch.randn(E, 1, generator=g))
    critic["v_out.weight"] = q.T.contiguous() * 0.01
    _, critic["v_out.bias"] = lin(1, E)
    return actor, critic


def random_parameters_central(self_dim, num_agents, seed=0):
    """`random_parameters` for critic_input: state: (the shared actor, the centralised critic — the encoder over state_drones / cylinders and
    v_out = Linear(128, num_agents), orthogonal with gain 0.01 —) in the reference's names, CPU fp32."""
    actor, obs_critic = random_parameters(self_dim, num_agents, seed)
    critic = {k.replace("state_self", "state_drones"): v for k, v in obs_critic.items() if "state_others" not in k and not k.startswith("v_out.")}
    g = torch.Generator().manual_seed(seed + 7919)
    q, _ = torch.linalg.qr(torch.randn(EMBED_DIM, num_agents, generator=g))
    critic["v_out.weight"] = q.T.contiguous() * 0.01
    critic["v_out.bias"] = (torch.rand(num_agents, generator=g) * 2 - 1) / math.sqrt(EMBED_DIM)
    return actor, critic


def random_parameters_per_agent(self_dim, num_agents, seed=0):
    """`random_parameters` for share_actor: False: (the stacked actor — `num_agents` independently initialised actors, every tensor
    [A, ...] — and the critic) in the reference's names, CPU fp32."""
    nets = [random_parameters(self_dim, num_agents, seed + 1000 * a) for a in range(num_agents)]
    return {k: torch.stack([n[0][k] for n in nets]).contiguous() for k in nets[0][0]}, nets[0][1]


def random_rnn_parameters_per_agent(num_agents, seed=0):
    """`random_rnn_parameters` for share_actor: False: `num_agents` independently initialised GRU blocks, every tensor [A, ...], under the
    reference's names with the `rnn.` prefix: merge it into `random_parameters_per_agent`'s stacked actor."""
    nets = [random_rnn_parameters(seed + 1000 * a) for a in range(num_agents)]
    return {k: torch.stack([n[k] for n in nets]).contiguous() for k in nets[0]}


# ---------------------------------------------------------------------------------------------------------------------------------------
# The eight C entries, keyed as kPolKernels of hns_policy.hip: (agents, rnn, act).  The four classes below are the four (agents, rnn) pairs.
ENTRIES = {
    (False, False, False): "hns_policy_forward", (False, False, True): "hns_policy_act",
    (False, True, False): "hns_policy_forward_rnn", (False, True, True): "hns_policy_act_rnn",
    (True, False, False): "hns_policy_forward_agents", (True, False, True): "hns_policy_act_agents",
    (True, True, False): "hns_policy_forward_rnn_agents", (True, True, True): "hns_policy_act_rnn_agents",
}
P_SCALE = 6 * EMBED_DIM * EMBED_DIM + 18 * EMBED_DIM + 4          # P_SCALE of hns_policy.hip: where exp(log_std) lies in an actor's image, in floats


class DevicePolicy:
    """The actor's and critic's forward pass of MAPPOPolicy (shared actor, critic on the observation) in one HIP launch per call.

    `DevicePolicy(actor_params, critic)`: actor_params a TensorDictParams / TensorDict / mapping / nn.Module of the actor's parameters,
    critic the critic TensorDictModule / nn.Module / state_dict.  Live tensors are read in place (an optimiser step is followed); anything on
    another device than `device` is copied once.  `cfg` (the algo cfg, optional) is checked for what this pass does not implement.

    This class holds everything the four configurations share, switched by two class attributes: `per_agent` (a stacked actor, `num_agents`
    slices) and `recurrent` (`actor_rnn` / `critic_rnn`, a GRU behind each encoder).  The subclasses set them, parse their parameters and
    adapt the arguments of `forward`, `act` and `act_step` to `_pass`."""
    per_agent = recurrent = central = False
    needs_state = False                                          # the collector hands ("agents", "state") to `forward` (the two central classes)
    actor_rnn = critic_rnn = None

    def __init__(self, actor_params, critic, cfg=None, device=None, seed=0, agent_name="drone"):
        check_config(cfg)
        self._setup(parse_parameters(actor_params, ACTOR_NAMES, "actor"), parse_parameters(critic, CRITIC_NAMES, "critic"), device, seed, agent_name)

    def _setup(self, actor_p, critic_p, device, seed, agent_name):
        """Everything behind the parsing: the device, the shapes the two networks must agree on, the packed images and the noise."""
        self.actor_p, self.critic_p = actor_p, critic_p
        ds = {v.device for v in (*self.actor_p.values(), *self.critic_p.values())}
        self.device = torch.device(device) if device is not None else next(iter(ds))
        if ds != {self.device}:
            self.actor_p = {k: v.detach().to(self.device).contiguous() for k, v in self.actor_p.items()}
            self.critic_p = {k: v.detach().to(self.device).contiguous() for k, v in self.critic_p.items()}
        self.self_dim = int(self.actor_p["embed_self_w"].shape[-1])
        if int(self.critic_p["embed_self_w"].shape[1]) != self.self_dim:
            raise PolicyConfigError("actor and critic see state_self rows of different widths")
        if not self.central and ("embed_others_w" in self.actor_p) != ("embed_others_w" in self.critic_p):
            raise PolicyConfigError("actor and critic disagree on the state_others key")
        self.has_others = "embed_others_w" in self.actor_p
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.agent_name = agent_name
        self._stamp = None
        self._generator = None
        if self.device.type == "cuda":
            self._lib = abi.load_library()
            self.packed = torch.empty(self._packed_bytes(), dtype=torch.uint8, device=self.device)
            self.counter = torch.zeros(1, dtype=torch.int64, device=self.device)   # the Philox call counter (uint64 on the device)
        else:
            self._generator = torch.Generator(device="cpu").manual_seed(self.seed)
        if self.recurrent:                                       # the GRU tensors on the policy's device and their packed image
            if {v.device for v in (*self.actor_rnn.values(), *self.critic_rnn.values())} != {self.device}:
                self.actor_rnn = {k: v.detach().to(self.device).contiguous() for k, v in self.actor_rnn.items()}
                self.critic_rnn = {k: v.detach().to(self.device).contiguous() for k, v in self.critic_rnn.items()}
            if self.device.type == "cuda":
                self.rnn_packed = torch.empty(self._rnn_packed_bytes(), dtype=torch.uint8, device=self.device)

    @classmethod
    def from_checkpoint(cls, checkpoint, cfg=None, device=None, seed=0):
        """From `MAPPOPolicy.state_dict()` (scripts/train.py:292,318) or a path to it: its "actor_params" and "critic" entries."""
        if not isinstance(checkpoint, dict):
            checkpoint = torch.load(checkpoint, map_location="cpu", weights_only=False)
        for k in ("actor_params", "critic"):
            if k not in checkpoint:
                raise KeyError(f"checkpoint has no {k!r} entry (keys: {sorted(checkpoint)})")
        return cls(checkpoint["actor_params"], checkpoint["critic"], cfg=cfg, device=device, seed=seed)

    # ---- packed images
    def _packed_bytes(self):
        if self.per_agent and self.central:
            return self._lib.hns_policy_packed_central_agents_bytes(self.self_dim, self.num_agents)
        if self.per_agent:
            return self._lib.hns_policy_packed_agents_bytes(self.self_dim, self.num_agents)
        if self.central:
            return self._lib.hns_policy_packed_central_bytes(self.self_dim, self.num_agents)
        return self._lib.hns_policy_packed_bytes(self.self_dim)

    def _pack_agents(self):
        """The pack entry's num_agents.  Of hns_policy_pack's only > 1 matters (the networks have the state_others embedding)."""
        return self.num_agents if self.per_agent or self.central else 2 if self.has_others else 1

    def _rnn_packed_bytes(self):
        return self._lib.hns_policy_rnn_packed_agents_bytes(self.num_agents) if self.per_agent else self._lib.hns_policy_rnn_packed_bytes()

    def _rnn_pack(self, a, c, st):
        """(return code, entry) of the GRU images' pack call."""
        if self.per_agent:
            return (self._lib.hns_policy_rnn_pack_agents(C.byref(a), C.byref(c), self.num_agents, self.rnn_packed.data_ptr(), st),
                    "hns_policy_rnn_pack_agents")
        return self._lib.hns_policy_rnn_pack(C.byref(a), C.byref(c), self.rnn_packed.data_ptr(), st), "hns_policy_rnn_pack"

    def _tensors(self):
        rnn = [*self.actor_rnn.values(), *self.critic_rnn.values()] if self.recurrent else []
        return [*self.actor_p.values(), *self.critic_p.values(), *rnn]

    def _net(self, p):
        n = abi.HnsPolicyNet()
        for f in abi.POLICY_NET_FIELDS:
            if f in p:
                if not p[f].is_contiguous():
                    raise ValueError(f"parameter {f} must be contiguous")
                setattr(n, f, p[f].data_ptr())
        return n

    def _gru_net(self, p):
        n = abi.HnsGruNet()
        for f, t in p.items():
            setattr(n, f, t.data_ptr())
        return n

    def refresh(self, force=False):
        """Re-pack the operand image — recurrent: both images — if a parameter's storage or version counter moved (or `force`)."""
        stamp = tuple((t.data_ptr(), t._version) for t in self._tensors())
        if not force and stamp == self._stamp:
            return
        pack = ("hns_policy_pack_central_agents" if self.per_agent and self.central else "hns_policy_pack_agents" if self.per_agent else
                "hns_policy_pack_central" if self.central else "hns_policy_pack")
        a, c = self._net(self.actor_p), self._net(self.critic_p)
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            self._check(getattr(self._lib, pack)(C.byref(a), C.byref(c), self.self_dim, self._pack_agents(), self.packed.data_ptr(), st), pack)
            if self.recurrent:
                self._check(*self._rnn_pack(self._gru_net(self.actor_rnn), self._gru_net(self.critic_rnn), st))
        self._stamp = stamp

    @property
    def scale(self):
        """exp(log_std) as the kernel uses it, [4] or (per_agent) [A, 4] (device: read from the packed image, the agents' images)."""
        if self.device.type != "cuda":
            return torch.exp(self.actor_p["log_std"].detach())
        self.refresh()
        img = self.packed.view(torch.float32)
        if self.per_agent:
            net = self._lib.hns_policy_packed_bytes(self.self_dim) // 8                 # one network's image, in floats: the actors' come first
            return img[:self.num_agents * net].view(self.num_agents, net)[:, P_SCALE:P_SCALE + ACTION_DIM]
        return img[P_SCALE:P_SCALE + ACTION_DIM]

    def _check(self, rc, what):
        if rc != abi.HNS_OK:
            raise RuntimeError(f"{what} failed ({rc}): {self._lib.hns_last_error().decode()}")

    # ---- the pass
    def _validate(self, xs, xo, xc):
        if xs.dim() == 4:
            if xs.shape[2] != 1:
                raise ValueError(f"state_self must be [E, A, D] or [E, A, 1, D], not {tuple(xs.shape)}")
            xs = xs.squeeze(2)
        if xs.dim() != 3 or xs.shape[-1] != self.self_dim:
            raise ValueError(f"state_self must be [E, A, {self.self_dim}], not {tuple(xs.shape)}")
        E, A, _ = xs.shape
        if (xo is not None) != self.has_others or (A > 1) != self.has_others:
            raise ValueError(f"{A} agents: state_others is {'required' if A > 1 else 'absent'} for this network")
        if xo is not None and (xo.dim() != 4 or tuple(xo.shape) != (E, A, A - 1, 3)):
            raise ValueError(f"state_others must be [{E}, {A}, {A - 1}, 3], not {tuple(xo.shape)}")
        if xc.dim() != 4 or tuple(xc.shape[:2]) != (E, A) or xc.shape[-1] != 5 or not 1 <= xc.shape[2] <= abi.HNS_MAX_CYLINDERS:
            raise ValueError(f"cylinders must be [{E}, {A}, K, 5] with K in [1, {abi.HNS_MAX_CYLINDERS}], not {tuple(xc.shape)}")
        for name, t in (("state_self", xs), ("state_others", xo), ("cylinders", xc)):
            if t is None:
                continue
            if t.dtype != torch.float32:
                raise TypeError(f"{name} must be float32, not {t.dtype}")
            if t.device != self.device:
                raise ValueError(f"{name} is on {t.device}, the policy on {self.device}")
        if self.per_agent and A != self.num_agents:
            raise ValueError(f"the observation has {A} agents, the policy {self.num_agents} actors")
        return xs, xo, xc

    @staticmethod
    def _io(xs, xo, xc):
        """The observation part of an hns_policy_io: the tensors (made contiguous in their last axis only) with their strides."""
        xs, xc = (t if t.stride(-1) == 1 else t.contiguous() for t in (xs, xc))
        if xo is not None and xo.stride(-1) != 1:
            xo = xo.contiguous()
        io = abi.HnsPolicyIo()
        io.obs_self, io.obs_cylinders = xs.data_ptr(), xc.data_ptr()
        io.obs_others = xo.data_ptr() if xo is not None else None
        io.self_stride[:] = [xs.stride(0), xs.stride(1)]
        io.others_stride[:] = [xo.stride(0), xo.stride(1), xo.stride(2)] if xo is not None else [0, 0, 0]
        io.cyl_stride[:] = [xc.stride(0), xc.stride(1), xc.stride(2)]
        return xs, xo, xc, io

    def _state(self, t, name, E, A):
        if t is None:
            return None
        if (not torch.is_tensor(t) or tuple(t.shape) != (E, A, EMBED_DIM) or t.dtype != torch.float32 or t.device != self.device
                or not t.is_contiguous() or (t.is_cuda and t.data_ptr() % 16)):
            raise ValueError(f"{name} must be a contiguous, 16-byte aligned float32 [{E}, {A}, {EMBED_DIM}] tensor on {self.device}")
        return t

    def _flags(self, is_init, E):
        """is_init as the kernels take it: uint8 [E], contiguous (None stays None)."""
        if is_init is None:
            return None
        if not torch.is_tensor(is_init) or is_init.numel() != E or is_init.device != self.device:
            raise ValueError(f"is_init must hold one flag per env ([{E}] or [{E}, 1]) on {self.device}")
        is_init = is_init.reshape(E).contiguous()                # (a time slice of a stored [N, T, 1] tensor is strided)
        return is_init.view(torch.uint8) if is_init.dtype == torch.bool else (is_init != 0).view(torch.uint8)

    def _pass(self, obs, act=False, eps=None, deterministic=False, value_only=False, out=None, states=None, is_init=None, state=None):
        """One call of ENTRIES[per_agent, recurrent, act] — on CPU tensors, of `_restatement` — as (action, log_prob, value, loc, actor_state,
        critic_state): what the pass does not compute is None.  obs: (state_self, state_others, cylinders).  act: the actor's half alone,
        the mode into `out` (or a fresh tensor), no noise, the call counter untouched.  states (recurrent): name -> tensor or None in the
        order (the actor's state, the critic's, the tensor the actor's new state is written into, the critic's), the names the caller's
        own for the refusals; act takes the actor's two.  state (central): (state_drones, state_cylinders) as `forward` takes them."""
        xs, xo, xc = self._validate(*obs)
        E, A, _ = xs.shape
        dev = self.device
        if self.central and not act:
            sd, sc = self._validate_state(*state, xc)
        if eps is not None and (tuple(eps.shape) != (E, A, ACTION_DIM) or eps.dtype != torch.float32 or eps.device != dev):
            raise ValueError(f"eps must be float32 [{E}, {A}, {ACTION_DIM}] on {dev}")
        ha = hc = oa = oc = None
        if self.recurrent:
            checked = [self._state(t, name, E, A) for name, t in states.items()]
            if act:
                ha, oa = checked
            else:
                ha, hc, oa, oc = checked
            is_init = self._flags(is_init, E)
        if out is not None and (tuple(out.shape) != (E, A, ACTION_DIM) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 [{E}, {A}, {ACTION_DIM}] tensor on {dev}")
        actor = act or not value_only                            # the actor's half runs: its state is read and written
        if dev.type != "cuda":
            if self.recurrent:
                # contiguous observations: torch's CPU matrix products round differently for strided operands, and a stored rollout re-run
                # from views of its storage must give the bits the collection gave.  The classes without a GRU never did this and still
                # do not: their CPU bits on strided observations are the strided products'.
                xs, xc, xo = xs.contiguous(), xc.contiguous(), (xo.contiguous() if xo is not None else None)
            if self.central and not act:
                with torch.no_grad():                            # (a contiguous state: a strided view of the env's cylinders rounds differently on the CPU)
                    return (*torch_forward_central(self.actor_p, self.critic_p, xs.unsqueeze(2), xo, xc, sd.contiguous(), sc.contiguous(), eps,
                                                   deterministic, value_only, self._generator, stacked=self.per_agent), None, None)
            with torch.no_grad():
                action, log_prob, value, loc, new_a, new_c = _restatement(
                    self.actor_p, self.critic_p, xs.unsqueeze(2), xo, xc, self.actor_rnn, self.critic_rnn, ha, hc, is_init, eps,
                    deterministic, value_only, self._generator, stacked=self.per_agent, actor_only=act)
            if out is not None:
                action = out.copy_(action)
            if oa is not None and actor:
                new_a = oa.copy_(new_a)
            if oc is not None:
                new_c = oc.copy_(new_c)
            return action, log_prob, value, loc, new_a, new_c
        self.refresh()
        xs, xo, xc, io = self._io(xs, xo, xc)
        action = log_prob = value = loc = None
        if actor:
            action = out if out is not None else torch.empty(E, A, ACTION_DIM, device=dev)
            io.action = action.data_ptr()
        if not act:
            value = torch.empty(E, A, 1, device=dev)
            io.value = value.data_ptr()
            if eps is not None:
                eps = eps.contiguous()                           # (held until the call below is enqueued)
                io.eps = eps.data_ptr()
            if actor:
                log_prob, loc = torch.empty(E, A, 1, device=dev), torch.empty(E, A, ACTION_DIM, device=dev)
                io.log_prob, io.loc = log_prob.data_ptr(), loc.data_ptr()
        args = [self.packed.data_ptr(), self.self_dim, E, A, xc.shape[2], C.byref(io)]
        if self.central and not act:
            sd, sc = (t if t.stride(-1) == 1 else t.contiguous() for t in (sd, sc))
            st = abi.HnsPolicyState()
            st.state_drones, st.cylinders = sd.data_ptr(), sc.data_ptr()
            st.drones_stride[:] = [sd.stride(0), sd.stride(1)]
            st.cyl_stride[:] = [sc.stride(0), sc.stride(1)]
            args.append(C.byref(st))
        if self.recurrent:
            rio = abi.HnsPolicyRnnIo()
            if actor:
                oa = oa if oa is not None else torch.empty(E, A, EMBED_DIM, device=dev)
                rio.actor_h_in, rio.actor_h_out = ha.data_ptr() if ha is not None else None, oa.data_ptr()
            else:
                oa = None
            if not act:
                oc = oc if oc is not None else torch.empty(E, A, EMBED_DIM, device=dev)
                rio.critic_h_in, rio.critic_h_out = hc.data_ptr() if hc is not None else None, oc.data_ptr()
            rio.is_init = is_init.data_ptr() if is_init is not None else None
            args.insert(1, self.rnn_packed.data_ptr())
            args.append(C.byref(rio))
        if not act:
            args += [(abi.HNS_POLICY_DETERMINISTIC if deterministic else 0) | (abi.HNS_POLICY_VALUE_ONLY if value_only else 0), self.seed,
                     self.counter.data_ptr()]
        entry = (("hns_policy_central_forward_agents" if self.per_agent else "hns_policy_central_forward") if self.central and not act else
                 ENTRIES[self.per_agent, self.recurrent, act])
        with torch.cuda.device(dev):
            rc = getattr(self._lib, entry)(*args, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        self._check(rc, entry)
        return action, log_prob, value, loc, oa, oc

    def forward(self, obs_self, obs_others, obs_cylinders, eps=None, deterministic=False, value_only=False):
        """PolicyOutput(action [E, A, 4], log_prob [E, A, 1], value [E, A, 1], loc [E, A, 4]); value_only: only value is set."""
        return PolicyOutput(*self._pass((obs_self, obs_others, obs_cylinders), eps=eps, deterministic=deterministic, value_only=value_only)[:4])

    def act(self, obs_self, obs_others, obs_cylinders, out=None):
        """The mode of the actor's distribution, action [E, A, 4], from the actor alone (hns_policy_act: one encoder pass, no critic, no
        log-prob, no noise, the call counter untouched) — bit for bit `forward(..., deterministic=True).action`.  `out`: a contiguous fp32
        [E, A, 4] tensor on the policy's device, written in place and returned (an evaluation loop's one action tensor)."""
        return self._pass((obs_self, obs_others, obs_cylinders), act=True, out=out)[0]

    @staticmethod
    def _obs(td):
        obs = td[("agents", "observation")]
        xo = obs.get("state_others", None) if hasattr(obs, "get") else None
        return obs["state_self"], xo, obs["cylinders"]

    def __call__(self, tensordict, deterministic=False):
        """MAPPOPolicy.__call__: writes ("agents", "action"), "<agent>.action_logp" and "state_value" into the tensordict and returns it."""
        out = self.forward(*self._obs(tensordict), deterministic=deterministic)
        tensordict[("agents", "action")] = out.action
        tensordict[f"{self.agent_name}.action_logp"] = out.log_prob
        tensordict["state_value"] = out.value
        return tensordict

    def value(self, tensordict):
        """value_op: the critic's state_value [E, A, 1] (train_op's next_value)."""
        return self.forward(*self._obs(tensordict), value_only=True).value


class PerAgentDevicePolicy(DevicePolicy):
    """MAPPOPolicy with share_actor: False — one actor per pursuer, the critic shared (the parameters stacked over the agents,
    mappo.py:148-152, the actor vmapped over the agent axis, mappo.py:243-246) — in one HIP launch per call.  DESIGN.md §7.16.

    `PerAgentDevicePolicy(actor_params, critic)`: actor_params the STACKED actor (TensorDictParams / TensorDict / mapping, every leaf
    [A, ...], as the reference's `actor_params`), critic as for DevicePolicy.  `forward`, `act`, `__call__` and `value` are DevicePolicy's,
    on `hns_policy_forward_agents` / `hns_policy_act_agents`: a tile is 32 envs of one agent and reads that agent's image, and row (e, a)
    is bit for bit DevicePolicy's with agent a's slice as the shared actor.  `scale` is [A, 4].  Refused with PolicyConfigError: whatever
    DevicePolicy refuses except share_actor: False; share_actor: True; tensors that are not stacked or whose leading sizes disagree; an
    observation with another number of agents (ValueError, as the other shape refusals)."""
    per_agent = True

    def __init__(self, actor_params, critic, cfg=None, device=None, seed=0, agent_name="drone"):
        check_config_per_agent(cfg)
        actor_p, self.num_agents = parse_parameters_per_agent(actor_params, "actor")
        self._setup(actor_p, parse_parameters(critic, CRITIC_NAMES, "critic"), device, seed, agent_name)


class RecurrentDevicePolicy(DevicePolicy):
    """MAPPOPolicy with actor.rnn / critic.rnn (a GRU(128, 128) behind each encoder) in one HIP launch per call: encoder -> GRU step -> head
    for both networks, the states read and written on the device.  Built from the same sources as DevicePolicy; the GRU tensors are the
    `rnn.*` entries of the actor's and the critic's parameters.  `forward` takes and returns the two states ([E, A, 128]; None: zeros) and
    an env-level `is_init` ([E] or [E, 1]; None: no env starts an episode); `out_states` may be the input tensors (in place).  `act_step` is
    the actor-only pass with the actor's state (evaluation); `act`, which has no state argument, keeps refusing."""
    recurrent = True

    def __init__(self, actor_params, critic, cfg=None, device=None, seed=0, agent_name="drone"):
        check_config(cfg_without(cfg, "actor.rnn", "critic.rnn"))
        actor_rest, self.actor_rnn = split_rnn(actor_params, "actor")
        critic_rest, self.critic_rnn = split_rnn(critic, "critic")
        self._setup(parse_parameters(actor_rest, ACTOR_NAMES, "actor"), parse_parameters(critic_rest, CRITIC_NAMES, "critic"), device, seed, agent_name)

    def act(self, *args, **kwargs):
        raise PolicyConfigError("a recurrent policy has no actor-only pass; use forward(..., deterministic=True)")

    def act_step(self, obs_self, obs_others, obs_cylinders, state=None, is_init=None, out=None, out_state=None):
        """The actor-only pass of a recurrent policy: (action [E, A, 4], state [E, A, 128]), the mode of the actor's distribution and the
        actor's state AFTER the step (hns_policy_act_rnn: the actor's encoder, GRU step and head; no critic, no log-prob, no noise, the call
        counter untouched) — bit for bit `forward(..., actor_state=state, is_init=is_init, deterministic=True)`'s action and actor_state.
        state: [E, A, 128] or None for zeros; is_init as `forward` takes it.  out / out_state: contiguous fp32 tensors written in place and
        returned; out_state may be `state` (an evaluation loop's one action and one state tensor)."""
        r = self._pass((obs_self, obs_others, obs_cylinders), act=True, out=out, states={"state": state, "out_state": out_state}, is_init=is_init)
        return r[0], r[4]

    def forward(self, obs_self, obs_others, obs_cylinders, actor_state=None, critic_state=None, is_init=None, eps=None, deterministic=False,
                value_only=False, out_states=None):
        """RecurrentPolicyOutput(action [E, A, 4], log_prob [E, A, 1], value [E, A, 1], loc [E, A, 4], actor_state, critic_state [E, A, 128]):
        the states AFTER the step.  value_only: only value and critic_state are set, the actor's state is neither read nor written.
        out_states: (actor, critic) tensors the new states are written into (either may be None: a fresh tensor)."""
        oa, oc = out_states if out_states is not None else (None, None)
        states = {"actor_state": actor_state, "critic_state": critic_state, "out_states[0]": oa, "out_states[1]": oc}
        return RecurrentPolicyOutput(*self._pass((obs_self, obs_others, obs_cylinders), eps=eps, deterministic=deterministic, value_only=value_only,
                                                 states=states, is_init=is_init))

    def _keys(self):
        return f"{self.agent_name}.actor_rnn_state", f"{self.agent_name}.critic_rnn_state"

    def __call__(self, tensordict, deterministic=False):
        """MAPPOPolicy.__call__ with rnn heads: reads "<agent>.actor_rnn_state", "<agent>.critic_rnn_state" (absent: zeros) and "is_init"
        (absent: none), writes the action, its log-prob, the value and — as the reference does — the states AFTER the step under the two
        state keys."""
        ka, kc = self._keys()
        out = self.forward(*self._obs(tensordict), actor_state=_td_get(tensordict, ka), critic_state=_td_get(tensordict, kc),
                           is_init=_td_get(tensordict, "is_init"), deterministic=deterministic)
        tensordict[("agents", "action")] = out.action
        tensordict[f"{self.agent_name}.action_logp"] = out.log_prob
        tensordict["state_value"] = out.value
        tensordict[ka], tensordict[kc] = out.actor_state, out.critic_state
        return tensordict

    def value(self, tensordict):
        """value_op: the critic's state_value [E, A, 1] from the tensordict's observation, critic state and is_init; nothing is written back."""
        return self.forward(*self._obs(tensordict), critic_state=_td_get(tensordict, self._keys()[1]), is_init=_td_get(tensordict, "is_init"),
                            value_only=True).value


class PerAgentRecurrentDevicePolicy(RecurrentDevicePolicy):
    """MAPPOPolicy with share_actor: False AND actor.rnn / critic.rnn — one actor and one actor GRU per pursuer (the stacked `actor_params`
    hold the actor's GRU too), the critic and its GRU shared — in one HIP launch per call (`hns_policy_forward_rnn_agents`; `act_step`:
    `hns_policy_act_rnn_agents`).  DESIGN.md §7.17.

    `PerAgentRecurrentDevicePolicy(actor_params, critic)`: actor_params the STACKED actor with its `rnn.*` leaves stacked too (every leaf
    [A, ...], as the reference's `actor_params` of this configuration), critic as for RecurrentDevicePolicy.  Every method is
    RecurrentDevicePolicy's over the agents' entries: a tile is 32 envs of one agent and reads that agent's two images, the states stay
    [E, A, 128], and row (e, a) is bit for bit RecurrentDevicePolicy's with agent a's slices as the shared actor.  `scale` is [A, 4].
    Refused with PolicyConfigError before anything is built: whatever RecurrentDevicePolicy refuses except share_actor: False;
    share_actor: True; tensors that are not stacked or whose leading sizes disagree; an rnn on only one of the two networks; a critic with
    stacked tensors; an observation with another number of agents (ValueError).  It is trained by
    learner.PerAgentRecurrentDeviceLearner."""
    per_agent = True

    def __init__(self, actor_params, critic, cfg=None, device=None, seed=0, agent_name="drone"):
        check_config_per_agent(cfg_without(cfg, "actor.rnn", "critic.rnn"))
        if is_stacked(critic, "base.attn.in_proj_weight"):
            raise PolicyConfigError("critic: parameters with a leading agent dimension; the reference stacks the actor only")
        actor_rest, self.actor_rnn, rnn_agents = split_rnn(actor_params, "actor", stacked=True)
        critic_rest, self.critic_rnn = split_rnn(critic, "critic")
        actor_p, self.num_agents = parse_parameters_per_agent(actor_rest, "actor")
        if rnn_agents != self.num_agents:
            raise PolicyConfigError(f"actor: {self.num_agents} stacked actors with {rnn_agents} stacked GRUs")
        self._setup(actor_p, parse_parameters(critic_rest, CRITIC_NAMES, "critic"), device, seed, agent_name)


class CentralCriticDevicePolicy(DevicePolicy):
    """MAPPOPolicy with critic_input: state — the shared actor on the observation and ONE centralised critic row per env (make_critic with
    centralized=True: the encoder over the state spec, the A rows of state_drones through one embedding, then the cylinders; v_out =
    Linear(128, A)) — in one HIP launch per call (`hns_policy_central_forward`: actor tiles of 32 (env, agent) rows beside critic tiles of
    32 envs).  DESIGN.md §7.20.

    `CentralCriticDevicePolicy(actor_params, critic)`: actor_params as for DevicePolicy, critic the centralised critic's 20 tensors under
    the reference's names (`base.split_embed.embed.state_drones.*`, `base.split_embed.embed.cylinders.*`, ..., `v_out.weight [A, 128]`).
    action, log_prob and loc are bit for bit DevicePolicy's for the same actor and noise; `act` (evaluation) is DevicePolicy's.  The state's
    cylinders: the reference's spec declares [E, K, 5] and its env returns [E, A, K, 5]; this class takes the declared shape and, from the
    env's tensor, agent 0's rows (the query drone's K nearest), read in place — a documented reading, not reference parity.  Refused with
    PolicyConfigError before anything is built: whatever DevicePolicy refuses except critic_input: state; critic_input: obs; stacked
    actors; an rnn; a critic with a state_others or state_self embedding; v_out with one row beside an actor with a state_others key (or
    several rows beside one without)."""
    central = True
    needs_state = True

    def __init__(self, actor_params, critic, cfg=None, device=None, seed=0, agent_name="drone"):
        check_config_central(cfg)
        actor_p = parse_parameters(actor_params, ACTOR_NAMES, "actor")
        critic_p, self.num_agents = parse_parameters_central(critic, "critic")
        if ("embed_others_w" in actor_p) != (self.num_agents > 1):
            raise PolicyConfigError(f"critic: v_out has {self.num_agents} row(s) but the actor has {'a' if 'embed_others_w' in actor_p else 'no'} "
                                    "state_others embedding (v_out is Linear(128, A) for A agents)")
        self._setup(actor_p, critic_p, device, seed, agent_name)

    def _validate_state(self, sd, sc, xc):
        """(state_drones [E, A, D], the state's cylinders [E, K, 5]) checked against the observation; sc None or [E, A, K, 5]: agent 0's rows."""
        E, A, K = xc.shape[:3]
        if A != self.num_agents:
            raise ValueError(f"the observation has {A} agents, v_out {self.num_agents} rows")
        if not torch.is_tensor(sd) or tuple(sd.shape) != (E, A, self.self_dim):
            raise ValueError(f"state_drones must be [{E}, {A}, {self.self_dim}], not {tuple(sd.shape) if torch.is_tensor(sd) else type(sd).__name__}")
        if sc is None:
            sc = xc
        if sc.dim() == 4 and tuple(sc.shape) == (E, A, K, 5):
            sc = sc[:, 0]                                        # the query drone's K nearest: a view, no copy
        if tuple(sc.shape) != (E, K, 5):
            raise ValueError(f"the state's cylinders must be [{E}, {K}, 5] or [{E}, {A}, {K}, 5], not {tuple(sc.shape)}")
        for name, t in (("state_drones", sd), ("the state's cylinders", sc)):
            if t.dtype != torch.float32:
                raise TypeError(f"{name} must be float32, not {t.dtype}")
            if t.device != self.device:
                raise ValueError(f"{name} is on {t.device}, the policy on {self.device}")
        return sd, sc

    def forward(self, obs_self, obs_others, obs_cylinders, state_drones, state_cylinders=None, eps=None, deterministic=False, value_only=False):
        """PolicyOutput(action [E, A, 4], log_prob [E, A, 1], value [E, A, 1], loc [E, A, 4]); value_only: only value is set (the critic
        workgroups alone).  state_drones [E, A, D]; state_cylinders [E, K, 5], the env's [E, A, K, 5] (agent 0's rows are read in place) or
        None: agent 0's rows of obs_cylinders, in place."""
        return PolicyOutput(*self._pass((obs_self, obs_others, obs_cylinders), eps=eps, deterministic=deterministic, value_only=value_only,
                                        state=(state_drones, state_cylinders))[:4])

    @staticmethod
    def _state_of(td):
        state = td[("agents", "state")]
        return state["state_drones"], state["cylinders"]

    def __call__(self, tensordict, deterministic=False):
        """MAPPOPolicy.__call__ with critic_input: state: the critic reads ("agents", "state")."""
        out = self.forward(*self._obs(tensordict), *self._state_of(tensordict), deterministic=deterministic)
        tensordict[("agents", "action")] = out.action
        tensordict[f"{self.agent_name}.action_logp"] = out.log_prob
        tensordict["state_value"] = out.value
        return tensordict

    def value(self, tensordict):
        """value_op: the critic's state_value [E, A, 1] from ("agents", "state")."""
        return self.forward(*self._obs(tensordict), *self._state_of(tensordict), value_only=True).value


class PerAgentCentralCriticDevicePolicy(CentralCriticDevicePolicy):
    """MAPPOPolicy with share_actor: False AND critic_input: state — one actor per pursuer on its own observation and ONE centralised critic
    row per env over the state: heterogeneous actors under one critic, centralised training with decentralised execution — in one HIP launch
    per call (`hns_policy_central_forward_agents`: per agent a range of actor tiles of 32 envs reading that agent's image, then the critic's
    range of tiles of 32 envs).  DESIGN.md §7.21.

    `PerAgentCentralCriticDevicePolicy(actor_params, critic)`: actor_params the STACKED actor as for PerAgentDevicePolicy (every leaf
    [A, ...]), critic the centralised critic's 20 tensors as for CentralCriticDevicePolicy; v_out's rows must equal the stacked leading size.
    `forward(obs_self, obs_others, obs_cylinders, state_drones, state_cylinders=None, ...)`, `__call__` and `value` are
    CentralCriticDevicePolicy's; `act` (`hns_policy_act_agents`, which this image serves unchanged) and `scale` [A, 4] are
    PerAgentDevicePolicy's.  action, log_prob and loc are bit for bit PerAgentDevicePolicy's for the same stacked actor and noise, value bit for
    bit CentralCriticDevicePolicy's for the same critic and state.  Refused with PolicyConfigError before anything is built: share_actor:
    True; critic_input: obs; an rnn; a tanh actor; actor tensors that are not stacked or whose leading sizes disagree; whatever
    CentralCriticDevicePolicy refuses of the critic; v_out with another number of rows than there are actors."""
    per_agent = True

    def __init__(self, actor_params, critic, cfg=None, device=None, seed=0, agent_name="drone"):
        check_config_per_agent_central(cfg)
        actor_p, self.num_agents = parse_parameters_per_agent(actor_params, "actor")
        critic_p, rows = parse_parameters_central(critic, "critic")
        if rows != self.num_agents:
            raise PolicyConfigError(f"critic: v_out has {rows} row(s) beside {self.num_agents} stacked actors (v_out is Linear(128, A) for A agents)")
        self._setup(actor_p, critic_p, device, seed, agent_name)
