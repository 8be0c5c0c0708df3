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
for bit `RecurrentDevicePolicy`'s with agent a's slices.  Collection and evaluation only: its update is an open item."""
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


def parse_parameters(params, names, what):
    """The hns_policy_net fields of one network from reference parameter names; raises PolicyConfigError on anything it does not implement."""
    flat = {_strip(k): v for k, v in _flatten(params).items()}
    out, unknown = {}, []
    for k, v in flat.items():
        if k in names:
            out[names[k]] = v
        else:
            unknown.append(k)
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
    if tuple(out["head_w"].shape) != (heads, E) or tuple(out["head_b"].shape) != (heads,):
        raise PolicyConfigError(f"{what}: the head must be Linear(128, {heads}), not {tuple(out['head_w'].shape)}")
    if heads == ACTION_DIM and tuple(out["log_std"].shape) != (ACTION_DIM,):
        raise PolicyConfigError(f"{what}: log_std must have {ACTION_DIM} values")
    if tuple(out["embed_cyl_w"].shape) != (E, 5):
        raise PolicyConfigError(f"{what}: the cylinders embedding must be Linear(5, 128)")
    if ("embed_others_w" in out) and tuple(out["embed_others_w"].shape) != (E, 3):
        raise PolicyConfigError(f"{what}: the state_others embedding must be Linear(3, 128)")
    sw = out["embed_self_w"]
    if sw.dim() != 2 or sw.shape[0] != E or not 1 <= sw.shape[1] <= abi.HNS_POLICY_MAX_SELF_DIM:
        raise PolicyConfigError(f"{what}: the state_self embedding must be Linear(D, 128) with D in [1, {abi.HNS_POLICY_MAX_SELF_DIM}]")
    for k, v in out.items():
        if v.dtype != torch.float32:
            raise TypeError(f"{what}: parameter {k} must be float32, not {v.dtype}")
    return out


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


def torch_forward(actor, critic, xs, xo, xc, eps=None, deterministic=False, value_only=False, generator=None):
    """The CPU path: (action, log_prob, value, loc) from parameter dicts in hns_policy_net field names; xs [E, A, 1, D]."""
    value = F.linear(_encoder(critic, xs, xo, xc), critic["head_w"], critic["head_b"])
    if value_only:
        return PolicyOutput(None, None, value, None)
    return PolicyOutput(*_heads(actor, _encoder(actor, xs, xo, xc), value, eps, deterministic, generator))


# ---------------------------------------------------------------------------------------------------------------------------------------
class DevicePolicy:
    """The actor's and critic's forward pass of MAPPOPolicy (shared actor, critic on the observation) in one HIP launch per call.

    `DevicePolicy(actor_params, critic)`: actor_params a TensorDictParams / TensorDict / mapping / nn.Module of the actor's parameters,
    critic the critic TensorDictModule / nn.Module / state_dict.  Live tensors are read in place (an optimiser step is followed); anything on
    another device than `device` is copied once.  `cfg` (the algo cfg, optional) is checked for what this pass does not implement."""

    def __init__(self, actor_params, critic, cfg=None, device=None, seed=0, agent_name="drone"):
        check_config(cfg)
        self._setup(parse_parameters(actor_params, ACTOR_NAMES, "actor"), parse_parameters(critic, CRITIC_NAMES, "critic"), device, seed, agent_name)

    def _setup(self, actor_p, critic_p, device, seed, agent_name):
        """Everything behind the parsing: the device, the shapes the two networks must agree on, the packed image and the noise."""
        self.actor_p, self.critic_p = actor_p, critic_p
        ds = {v.device for v in (*self.actor_p.values(), *self.critic_p.values())}
        self.device = torch.device(device) if device is not None else next(iter(ds))
        if ds != {self.device}:
            self.actor_p = {k: v.detach().to(self.device).contiguous() for k, v in self.actor_p.items()}
            self.critic_p = {k: v.detach().to(self.device).contiguous() for k, v in self.critic_p.items()}
        self.self_dim = int(self.actor_p["embed_self_w"].shape[-1])
        if int(self.critic_p["embed_self_w"].shape[1]) != self.self_dim:
            raise PolicyConfigError("actor and critic see state_self rows of different widths")
        if ("embed_others_w" in self.actor_p) != ("embed_others_w" in self.critic_p):
            raise PolicyConfigError("actor and critic disagree on the state_others key")
        self.has_others = "embed_others_w" in self.actor_p
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.agent_name = agent_name
        self._stamp = None
        self._generator = None
        if self.device.type == "cuda":
            self._lib = abi.load_library()
            nbytes = self._packed_bytes()
            self.packed = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.counter = torch.zeros(1, dtype=torch.int64, device=self.device)   # the Philox call counter (uint64 on the device)
        else:
            self._generator = torch.Generator(device="cpu").manual_seed(self.seed)

    @classmethod
    def from_checkpoint(cls, checkpoint, cfg=None, device=None, seed=0):
        """From `MAPPOPolicy.state_dict()` (scripts/train.py:292,318) or a path to it: its "actor_params" and "critic" entries."""
        if not isinstance(checkpoint, dict):
            checkpoint = torch.load(checkpoint, map_location="cpu", weights_only=False)
        for k in ("actor_params", "critic"):
            if k not in checkpoint:
                raise KeyError(f"checkpoint has no {k!r} entry (keys: {sorted(checkpoint)})")
        return cls(checkpoint["actor_params"], checkpoint["critic"], cfg=cfg, device=device, seed=seed)

    # ---- packed image
    _PACK, _FORWARD, _ACT = "hns_policy_pack", "hns_policy_forward", "hns_policy_act"     # the C entries (PerAgentDevicePolicy: the *_agents ones)

    def _packed_bytes(self):
        return self._lib.hns_policy_packed_bytes(self.self_dim)

    def _pack_agents(self):
        """hns_policy_pack's num_agents: only > 1 matters (the networks have the state_others embedding)."""
        return 2 if self.has_others else 1

    def _cpu_forward(self, xs, xo, xc, eps=None, deterministic=False, value_only=False):
        return torch_forward(self.actor_p, self.critic_p, xs.unsqueeze(2), xo, xc, eps, deterministic, value_only, self._generator)

    def _tensors(self):
        return [*self.actor_p.values(), *self.critic_p.values()]

    def _net(self, p):
        n = abi.HnsPolicyNet()
        for f in abi.POLICY_NET_FIELDS:
            if f in p:
                if not p[f].is_contiguous():
                    raise ValueError(f"parameter {f} must be contiguous")
                setattr(n, f, p[f].data_ptr())
        return n

    def refresh(self, force=False):
        """Re-pack the operand image if a parameter's storage or version counter moved (or `force`)."""
        stamp = tuple((t.data_ptr(), t._version) for t in self._tensors())
        if not force and stamp == self._stamp:
            return
        a, c = self._net(self.actor_p), self._net(self.critic_p)
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            rc = getattr(self._lib, self._PACK)(C.byref(a), C.byref(c), self.self_dim, self._pack_agents(), self.packed.data_ptr(), st)
        self._check(rc, self._PACK)
        self._stamp = stamp

    @property
    def scale(self):
        """exp(log_std) as the kernel uses it (device: read from the packed image)."""
        if self.device.type != "cuda":
            return torch.exp(self.actor_p["log_std"].detach())
        self.refresh()
        img = self.packed.view(torch.float32)
        off = 6 * EMBED_DIM * EMBED_DIM + 18 * EMBED_DIM + 4          # P_SCALE of hns_policy.hip
        return img[off:off + ACTION_DIM]

    def _check(self, rc, what):
        if rc != abi.HNS_OK:
            raise RuntimeError(f"{what} failed ({rc}): {self._lib.hns_last_error().decode()}")

    # ---- forward
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

    def forward(self, obs_self, obs_others, obs_cylinders, eps=None, deterministic=False, value_only=False):
        """PolicyOutput(action [E, A, 4], log_prob [E, A, 1], value [E, A, 1], loc [E, A, 4]); value_only: only value is set."""
        xs, xo, xc = self._validate(obs_self, obs_others, obs_cylinders)
        E, A, D = xs.shape
        if eps is not None and (tuple(eps.shape) != (E, A, ACTION_DIM) or eps.dtype != torch.float32 or eps.device != self.device):
            raise ValueError(f"eps must be float32 [{E}, {A}, {ACTION_DIM}] on {self.device}")
        if self.device.type != "cuda":
            with torch.no_grad():
                return self._cpu_forward(xs, xo, xc, eps, deterministic, value_only)
        self.refresh()
        xs, xo, xc, io = self._io(xs, xo, xc)
        eps = eps.contiguous() if eps is not None else None
        dev = self.device
        value = torch.empty(E, A, 1, device=dev)
        action = log_prob = loc = None
        if not value_only:
            action, log_prob, loc = torch.empty(E, A, ACTION_DIM, device=dev), torch.empty(E, A, 1, device=dev), torch.empty(E, A, ACTION_DIM, device=dev)
        io.eps = eps.data_ptr() if eps is not None else None
        io.value = value.data_ptr()
        if not value_only:
            io.action, io.log_prob, io.loc = action.data_ptr(), log_prob.data_ptr(), loc.data_ptr()
        flags = (abi.HNS_POLICY_DETERMINISTIC if deterministic else 0) | (abi.HNS_POLICY_VALUE_ONLY if value_only else 0)
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            rc = getattr(self._lib, self._FORWARD)(self.packed.data_ptr(), self.self_dim, E, A, xc.shape[2], C.byref(io), flags, self.seed,
                                                   self.counter.data_ptr(), st)
        self._check(rc, self._FORWARD)
        return PolicyOutput(action, log_prob, value, loc)

    def act(self, obs_self, obs_others, obs_cylinders, out=None):
        """The mode of the actor's distribution, action [E, A, 4], from the actor alone (hns_policy_act: one encoder pass, no critic, no
        log-prob, no noise, the call counter untouched) — bit for bit `forward(..., deterministic=True).action`.  `out`: a contiguous fp32
        [E, A, 4] tensor on the policy's device, written in place and returned (an evaluation loop's one action tensor)."""
        xs, xo, xc = self._validate(obs_self, obs_others, obs_cylinders)
        E, A, _ = xs.shape
        if out is not None and (tuple(out.shape) != (E, A, ACTION_DIM) or out.dtype != torch.float32 or out.device != self.device
                                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 [{E}, {A}, {ACTION_DIM}] tensor on {self.device}")
        if self.device.type != "cuda":
            with torch.no_grad():
                action = self._cpu_forward(xs, xo, xc, deterministic=True).action
            return action if out is None else out.copy_(action)
        self.refresh()
        xs, xo, xc, io = self._io(xs, xo, xc)
        action = out if out is not None else torch.empty(E, A, ACTION_DIM, device=self.device)
        io.action = action.data_ptr()
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            rc = getattr(self._lib, self._ACT)(self.packed.data_ptr(), self.self_dim, E, A, xc.shape[2], C.byref(io), st)
        self._check(rc, self._ACT)
        return action

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


# ---------------------------------------------------------------------------------------------------------------------------------------
# one actor per agent (share_actor: False): the parameters stacked over the agents (mappo.py:148-152), the actor vmapped over the agent axis
# (mappo.py:243-246); the critic stays shared.  DESIGN.md §7.16
def parse_parameters_per_agent(params, what="actor"):
    """(the hns_policy_net fields of the STACKED actor, every tensor [A, ...]; A) from reference parameter names.  Each agent's slice is held
    to `parse_parameters`' checks; tensors that are not stacked, or whose leading sizes disagree, raise PolicyConfigError."""
    flat = {_strip(k): v for k, v in _flatten(params).items()}
    w = flat.get("encoder.attn.in_proj_weight")
    if w is not None and w.dim() == 2:
        raise PolicyConfigError(f"{what}: the parameters have no leading agent dimension (a shared actor is DevicePolicy's)")
    sizes = {int(v.shape[0]) if v.dim() else None for v in flat.values()}
    if len(sizes) != 1 or None in sizes:
        raise PolicyConfigError(f"{what}: every stacked tensor needs the same leading agent dimension, not {sorted(str(s) for s in sizes)}")
    A = sizes.pop()
    if not 1 <= A <= abi.HNS_MAX_AGENTS:
        raise PolicyConfigError(f"{what}: {A} stacked actors outside [1, {abi.HNS_MAX_AGENTS}]")
    first = parse_parameters({k: v[0] for k, v in flat.items()}, ACTOR_NAMES, what)      # names, shapes, dtypes: every slice has slice 0's
    if ("embed_others_w" in first) != (A > 1):
        raise PolicyConfigError(f"{what}: {A} stacked actors {'need' if A > 1 else 'have no'} state_others embedding")
    return {ACTOR_NAMES[k]: v for k, v in flat.items()}, A


def agent_slice(actor_p, a):
    """Agent a's network out of the stacked one: views, a `parse_parameters` dict of its own."""
    return {k: v[a] for k, v in actor_p.items()}


def torch_forward_per_agent(actors, critic, xs, xo, xc, eps=None, deterministic=False, value_only=False, generator=None):
    """The CPU path of PerAgentDevicePolicy: `torch_forward` with the stacked actor — a loop over the agents' slices through `_encoder` and
    `_heads`.  Each slice runs on the WHOLE observation and keeps its own agent's rows, so agent a's rows are exactly `torch_forward`'s with
    slice a as the shared actor (a CPU matrix product's bits depend on its shape; this path serves tests, not speed)."""
    value = F.linear(_encoder(critic, xs, xo, xc), critic["head_w"], critic["head_b"])
    if value_only:
        return PolicyOutput(None, None, value, None)
    E, A = xs.shape[:2]
    if eps is None and not deterministic:
        eps = torch.randn((E, A, ACTION_DIM), dtype=xs.dtype, device=xs.device, generator=generator)
    rows = []
    for a in range(A):
        p = agent_slice(actors, a)
        rows.append([t[:, a:a + 1] for t in _heads(p, _encoder(p, xs, xo, xc), value, eps, deterministic, generator)])
    action, log_prob, _, loc = (torch.cat(t, dim=1) for t in zip(*rows))
    return PolicyOutput(action, log_prob, value, loc)


def check_config_per_agent(cfg):
    """`check_config` for one actor per agent: everything it refuses but share_actor: False; share_actor: True is refused instead."""
    if getter(cfg)("share_actor", False):
        raise PolicyConfigError("share_actor: True with one actor per agent; the shared actor is DevicePolicy's")
    check_config(cfg_without(cfg, "share_actor"))


class PerAgentDevicePolicy(DevicePolicy):
    """MAPPOPolicy with share_actor: False — one actor per pursuer, the critic shared — in one HIP launch per call.

    `PerAgentDevicePolicy(actor_params, critic)`: actor_params the STACKED actor (TensorDictParams / TensorDict / mapping, every leaf
    [A, ...], as the reference's `actor_params`), critic as for DevicePolicy.  `forward`, `act`, `__call__` and `value` are DevicePolicy's,
    on `hns_policy_forward_agents` / `hns_policy_act_agents`: a tile is 32 envs of one agent and reads that agent's image, and row (e, a)
    is bit for bit DevicePolicy's with agent a's slice as the shared actor.  `scale` is [A, 4].  Refused with PolicyConfigError: whatever
    DevicePolicy refuses except share_actor: False; share_actor: True; tensors that are not stacked or whose leading sizes disagree; an
    observation with another number of agents (ValueError, as the other shape refusals)."""
    per_agent = True
    _PACK, _FORWARD, _ACT = "hns_policy_pack_agents", "hns_policy_forward_agents", "hns_policy_act_agents"

    def __init__(self, actor_params, critic, cfg=None, device=None, seed=0, agent_name="drone"):
        check_config_per_agent(cfg)
        actor_p, self.num_agents = parse_parameters_per_agent(actor_params, "actor")
        self._setup(actor_p, parse_parameters(critic, CRITIC_NAMES, "critic"), device, seed, agent_name)

    def _packed_bytes(self):
        return self._lib.hns_policy_packed_agents_bytes(self.self_dim, self.num_agents)

    def _pack_agents(self):
        return self.num_agents

    def _cpu_forward(self, xs, xo, xc, eps=None, deterministic=False, value_only=False):
        return torch_forward_per_agent(self.actor_p, self.critic_p, xs.unsqueeze(2), xo, xc, eps, deterministic, value_only, self._generator)

    def _validate(self, xs, xo, xc):
        xs, xo, xc = super()._validate(xs, xo, xc)
        if xs.shape[1] != self.num_agents:
            raise ValueError(f"the observation has {xs.shape[1]} agents, the policy {self.num_agents} actors")
        return xs, xo, xc

    @property
    def scale(self):
        """exp(log_std) per agent, [A, 4], as the kernel uses it (device: read from the agents' packed images)."""
        if self.device.type != "cuda":
            return torch.exp(self.actor_p["log_std"].detach())
        self.refresh()
        img = self.packed.view(torch.float32).view(self.num_agents + 1, -1)
        off = 6 * EMBED_DIM * EMBED_DIM + 18 * EMBED_DIM + 4          # P_SCALE of hns_policy.hip
        return img[:self.num_agents, off:off + ACTION_DIM]


def random_parameters_per_agent(self_dim, num_agents, seed=0):
    """`random_parameters` for share_actor: False: (the stacked actor — `num_agents` independently initialised actors, every tensor
    [A, ...] — and the critic) in the reference's names, CPU fp32."""
    nets = [random_parameters(self_dim, num_agents, seed + 1000 * a) for a in range(num_agents)]
    return {k: torch.stack([n[0][k] for n in nets]).contiguous() for k in nets[0][0]}, nets[0][1]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the recurrent configuration (actor.rnn / critic.rnn): Actor.forward / Critic.forward with self.rnn set (mappo.py:603-660)
def _heads(actor, y_actor, value, eps, deterministic, generator):
    """(action, log_prob, value, loc) of the DiagGaussian head on the actor's features."""
    loc = F.linear(y_actor, actor["head_w"], actor["head_b"])
    scale = torch.broadcast_to(torch.exp(actor["log_std"]), loc.shape)
    if deterministic:
        action = loc
    else:
        if eps is None:
            eps = torch.randn(loc.shape, dtype=loc.dtype, device=loc.device, generator=generator)
        action = loc + scale * eps
    log_prob = torch.distributions.Normal(loc, scale).log_prob(action).sum(-1, keepdim=True)
    return action, log_prob, value, loc


def _rnn_step(p, rnn_p, xs, xo, xc, state, is_init):
    """One network's (LayerNorm(h' + f) [E, A, 128], h' [E, A, 128]): `_encoder`, then rnn.restatement over one step."""
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


def torch_forward_rnn(actor, critic, actor_rnn, critic_rnn, xs, xo, xc, actor_state=None, critic_state=None, is_init=None, eps=None,
                      deterministic=False, value_only=False, generator=None):
    """The CPU restatement of hns_policy_forward_rnn, any dtype: parameter dicts in hns_policy_net / hns_gru_net field names, xs [E, A, 1, D],
    states [E, A, 128] or None (zeros), is_init [E] (or [E, 1]) or None -> RecurrentPolicyOutput."""
    yc, hc = _rnn_step(critic, critic_rnn, xs, xo, xc, critic_state, is_init)
    value = F.linear(yc, critic["head_w"], critic["head_b"])
    if value_only:
        return RecurrentPolicyOutput(None, None, value, None, None, hc)
    ya, ha = _rnn_step(actor, actor_rnn, xs, xo, xc, actor_state, is_init)
    return RecurrentPolicyOutput(*_heads(actor, ya, value, eps, deterministic, generator), ha, hc)


def torch_act_rnn(actor, actor_rnn, xs, xo, xc, state=None, is_init=None):
    """The CPU restatement of hns_policy_act_rnn: the actor's half of `torch_forward_rnn` alone -> (loc [E, A, 4], the actor's state after the
    step [E, A, 128]); the same statements on the same operands, so the same bits as its deterministic action and actor_state."""
    ya, ha = _rnn_step(actor, actor_rnn, xs, xo, xc, state, is_init)
    return F.linear(ya, actor["head_w"], actor["head_b"]), ha


def _split_rnn_names(params, what):
    """(the parameters outside `rnn.`, the ones under it by their name behind `rnn.`), the latter held to the GRU block's six names."""
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
    return rest, found


def split_rnn(params, what):
    """(the network's parameters without its GRU, the GRU's six tensors by hns_gru_net field) from reference names: the GRU sits under
    `rnn.` (rnn.cell.weight_ih, ..., rnn.layer_norm.bias)."""
    from . import rnn as _rnn
    rest, found = _split_rnn_names(params, what)
    try:
        gru = _rnn.gru_parameters({_rnn.NAMES[k]: (v if v.is_contiguous() else v.detach().contiguous()) for k, v in found.items()})
    except ValueError as e:
        raise PolicyConfigError(f"{what}: the rnn must be GRUCell(128, 128) + LayerNorm(128): {e}") from None
    return rest, gru


class RecurrentDevicePolicy(DevicePolicy):
    """MAPPOPolicy with actor.rnn / critic.rnn (a GRU(128, 128) behind each encoder) in one HIP launch per call: encoder -> GRU step -> head
    for both networks, the states read and written on the device.  Built from the same sources as DevicePolicy; the GRU tensors are the
    `rnn.*` entries of the actor's and the critic's parameters.  `forward` takes and returns the two states ([E, A, 128]; None: zeros) and
    an env-level `is_init` ([E] or [E, 1]; None: no env starts an episode); `out_states` may be the input tensors (in place).  `act_step` is
    the actor-only pass with the actor's state (evaluation); `act`, which has no state argument, keeps refusing."""
    recurrent = True
    # the C entries of the recurrent pass (PerAgentRecurrentDevicePolicy: the *_agents ones)
    _FORWARD_RNN, _ACT_RNN = "hns_policy_forward_rnn", "hns_policy_act_rnn"

    def __init__(self, actor_params, critic, cfg=None, device=None, seed=0, agent_name="drone"):
        check_config(cfg_without(cfg, "actor.rnn", "critic.rnn"))
        actor_rest, self.actor_rnn = split_rnn(actor_params, "actor")
        critic_rest, self.critic_rnn = split_rnn(critic, "critic")
        super().__init__(actor_rest, critic_rest, cfg=None, device=device, seed=seed, agent_name=agent_name)
        self._setup_rnn()

    def _setup_rnn(self):
        """Behind `_setup`: the GRU tensors on the policy's device and their packed image."""
        if {v.device for v in (*self.actor_rnn.values(), *self.critic_rnn.values())} != {self.device}:
            self.actor_rnn = {k: v.detach().to(self.device).contiguous() for k, v in self.actor_rnn.items()}
            self.critic_rnn = {k: v.detach().to(self.device).contiguous() for k, v in self.critic_rnn.items()}
        if self.device.type == "cuda":
            self.rnn_packed = torch.empty(self._rnn_packed_bytes(), dtype=torch.uint8, device=self.device)

    def _rnn_packed_bytes(self):
        return self._lib.hns_policy_rnn_packed_bytes()

    def _rnn_pack(self, a, c, st):
        """(return code, entry) of the GRU images' pack call."""
        return self._lib.hns_policy_rnn_pack(C.byref(a), C.byref(c), self.rnn_packed.data_ptr(), st), "hns_policy_rnn_pack"

    def _cpu_forward_rnn(self, *args):
        return torch_forward_rnn(self.actor_p, self.critic_p, self.actor_rnn, self.critic_rnn, *args)

    def _cpu_act_rnn(self, *args):
        return torch_act_rnn(self.actor_p, self.actor_rnn, *args)

    def _tensors(self):
        return [*super()._tensors(), *self.actor_rnn.values(), *self.critic_rnn.values()]

    def _gru_net(self, p):
        n = abi.HnsGruNet()
        for f, t in p.items():
            setattr(n, f, t.data_ptr())
        return n

    def refresh(self, force=False):
        """Re-pack both images if a parameter's storage or version counter moved (or `force`)."""
        stamp = tuple((t.data_ptr(), t._version) for t in self._tensors())
        if not force and stamp == self._stamp:
            return
        super().refresh(force=True)
        a, c = self._gru_net(self.actor_rnn), self._gru_net(self.critic_rnn)
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            rc, entry = self._rnn_pack(a, c, st)
        self._check(rc, entry)
        self._stamp = stamp

    def act(self, *args, **kwargs):
        raise PolicyConfigError("a recurrent policy has no actor-only pass; use forward(..., deterministic=True)")

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

    def act_step(self, obs_self, obs_others, obs_cylinders, state=None, is_init=None, out=None, out_state=None):
        """The actor-only pass of a recurrent policy: (action [E, A, 4], state [E, A, 128]), the mode of the actor's distribution and the
        actor's state AFTER the step (hns_policy_act_rnn: the actor's encoder, GRU step and head; no critic, no log-prob, no noise, the call
        counter untouched) — bit for bit `forward(..., actor_state=state, is_init=is_init, deterministic=True)`'s action and actor_state.
        state: [E, A, 128] or None for zeros; is_init as `forward` takes it.  out / out_state: contiguous fp32 tensors written in place and
        returned; out_state may be `state` (an evaluation loop's one action and one state tensor)."""
        xs, xo, xc = self._validate(obs_self, obs_others, obs_cylinders)
        E, A, _ = xs.shape
        h, oh = self._state(state, "state", E, A), self._state(out_state, "out_state", E, A)
        is_init = self._flags(is_init, E)
        if out is not None and (tuple(out.shape) != (E, A, ACTION_DIM) or out.dtype != torch.float32 or out.device != self.device
                                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 [{E}, {A}, {ACTION_DIM}] tensor on {self.device}")
        if self.device.type != "cuda":
            xs, xc, xo = xs.contiguous(), xc.contiguous(), (xo.contiguous() if xo is not None else None)      # as forward: the same bits
            with torch.no_grad():
                action, new = self._cpu_act_rnn(xs.unsqueeze(2), xo, xc, h, is_init)
            return (action if out is None else out.copy_(action)), (new if oh is None else oh.copy_(new))
        self.refresh()
        xs, xo, xc, io = self._io(xs, xo, xc)
        action = out if out is not None else torch.empty(E, A, ACTION_DIM, device=self.device)
        oh = oh if oh is not None else torch.empty(E, A, EMBED_DIM, device=self.device)
        io.action = action.data_ptr()
        rio = abi.HnsPolicyRnnIo()
        rio.actor_h_in = h.data_ptr() if h is not None else None
        rio.actor_h_out = oh.data_ptr()
        rio.is_init = is_init.data_ptr() if is_init is not None else None
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            rc = getattr(self._lib, self._ACT_RNN)(self.packed.data_ptr(), self.rnn_packed.data_ptr(), self.self_dim, E, A, xc.shape[2], C.byref(io),
                                                   C.byref(rio), st)
        self._check(rc, self._ACT_RNN)
        return action, oh

    def forward(self, obs_self, obs_others, obs_cylinders, actor_state=None, critic_state=None, is_init=None, eps=None, deterministic=False,
                value_only=False, out_states=None):
        """RecurrentPolicyOutput(action [E, A, 4], log_prob [E, A, 1], value [E, A, 1], loc [E, A, 4], actor_state, critic_state [E, A, 128]):
        the states AFTER the step.  value_only: only value and critic_state are set, the actor's state is neither read nor written.
        out_states: (actor, critic) tensors the new states are written into (either may be None: a fresh tensor)."""
        xs, xo, xc = self._validate(obs_self, obs_others, obs_cylinders)
        E, A, D = xs.shape
        if eps is not None and (tuple(eps.shape) != (E, A, ACTION_DIM) or eps.dtype != torch.float32 or eps.device != self.device):
            raise ValueError(f"eps must be float32 [{E}, {A}, {ACTION_DIM}] on {self.device}")
        ha, hc = self._state(actor_state, "actor_state", E, A), self._state(critic_state, "critic_state", E, A)
        oa, oc = out_states if out_states is not None else (None, None)
        oa, oc = self._state(oa, "out_states[0]", E, A), self._state(oc, "out_states[1]", E, A)
        is_init = self._flags(is_init, E)
        if self.device.type != "cuda":
            # contiguous observations: torch's CPU matrix products round differently for strided operands, and a stored rollout re-run from
            # views of its storage must give the bits the collection gave
            xs, xc, xo = xs.contiguous(), xc.contiguous(), (xo.contiguous() if xo is not None else None)
            with torch.no_grad():
                out = self._cpu_forward_rnn(xs.unsqueeze(2), xo, xc, ha, hc, is_init, eps, deterministic, value_only, self._generator)
            new_a = out.actor_state if oa is None or value_only else oa.copy_(out.actor_state)
            new_c = out.critic_state if oc is None else oc.copy_(out.critic_state)
            return out._replace(actor_state=new_a, critic_state=new_c)
        self.refresh()
        xs, xo, xc, io = self._io(xs, xo, xc)
        eps = eps.contiguous() if eps is not None else None
        dev = self.device
        value = torch.empty(E, A, 1, device=dev)
        action = log_prob = loc = None
        oc = oc if oc is not None else torch.empty(E, A, EMBED_DIM, device=dev)
        if value_only:
            oa = None
        else:
            action, log_prob, loc = torch.empty(E, A, ACTION_DIM, device=dev), torch.empty(E, A, 1, device=dev), torch.empty(E, A, ACTION_DIM, device=dev)
            oa = oa if oa is not None else torch.empty(E, A, EMBED_DIM, device=dev)
            io.action, io.log_prob, io.loc = action.data_ptr(), log_prob.data_ptr(), loc.data_ptr()
        io.eps = eps.data_ptr() if eps is not None else None
        io.value = value.data_ptr()
        rio = abi.HnsPolicyRnnIo()
        rio.actor_h_in = ha.data_ptr() if ha is not None and not value_only else None
        rio.critic_h_in = hc.data_ptr() if hc is not None else None
        rio.actor_h_out = oa.data_ptr() if oa is not None else None
        rio.critic_h_out = oc.data_ptr()
        rio.is_init = is_init.data_ptr() if is_init is not None else None
        flags = (abi.HNS_POLICY_DETERMINISTIC if deterministic else 0) | (abi.HNS_POLICY_VALUE_ONLY if value_only else 0)
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            rc = getattr(self._lib, self._FORWARD_RNN)(self.packed.data_ptr(), self.rnn_packed.data_ptr(), self.self_dim, E, A, xc.shape[2],
                                                       C.byref(io), C.byref(rio), flags, self.seed, self.counter.data_ptr(), st)
        self._check(rc, self._FORWARD_RNN)
        return RecurrentPolicyOutput(action, log_prob, value, loc, oa, oc)

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


# ---------------------------------------------------------------------------------------------------------------------------------------
# one RECURRENT actor per agent (share_actor: False with actor.rnn / critic.rnn): the stacked `actor_params` hold the actor's GRU too, so
# every agent has an encoder, a GRU and a head of its own; the critic and the critic's GRU stay shared.  DESIGN.md §7.17
def is_stacked(params, name="encoder.attn.in_proj_weight"):
    """Whether `params` (any source `parse_parameters` reads) holds the stacked actor of share_actor: False: its in_proj_weight is [A, 384, 128]."""
    if params is None:
        return False
    w = {_strip(k): v for k, v in _flatten(params).items()}.get(name)
    return w is not None and w.dim() == 3


def split_rnn_per_agent(params, what="actor"):
    """`split_rnn` for the stacked actor: (the stacked parameters without the GRUs, the GRUs' six STACKED tensors by hns_gru_net field — every
    one [A, ...], contiguous —, A).  Each agent's slice is held to `gru_parameters`' checks; rnn tensors that are not stacked, or whose
    leading sizes disagree, raise PolicyConfigError."""
    from . import rnn as _rnn
    rest, found = _split_rnn_names(params, what)
    if any(v.dim() != (3 if k.endswith("weight_ih") or k.endswith("weight_hh") else 2) for k, v in found.items()):
        raise PolicyConfigError(f"{what}: the rnn tensors have no leading agent dimension (a shared recurrent actor is RecurrentDevicePolicy's)")
    sizes = {int(v.shape[0]) for v in found.values()}
    if len(sizes) != 1:
        raise PolicyConfigError(f"{what}: every stacked rnn tensor needs the same leading agent dimension, not {sorted(sizes)}")
    A = sizes.pop()
    if not 1 <= A <= abi.HNS_MAX_AGENTS:
        raise PolicyConfigError(f"{what}: {A} stacked GRUs outside [1, {abi.HNS_MAX_AGENTS}]")
    gru = {_rnn.NAMES[k]: (v if v.is_contiguous() else v.detach().contiguous()) for k, v in found.items()}
    for a in range(A):
        try:
            _rnn.gru_parameters({f: v[a] for f, v in gru.items()})
        except ValueError as e:
            raise PolicyConfigError(f"{what}: agent {a}'s rnn must be GRUCell(128, 128) + LayerNorm(128): {e}") from None
    return rest, {f: gru[f] for f in _rnn.FIELDS}, A


def torch_forward_rnn_per_agent(actors, critic, actor_rnns, critic_rnn, xs, xo, xc, actor_state=None, critic_state=None, is_init=None, eps=None,
                                deterministic=False, value_only=False, generator=None):
    """The CPU path of PerAgentRecurrentDevicePolicy: `torch_forward_rnn` with the stacked actor and the stacked actor GRU — a loop over the
    agents' slices, as `torch_forward_per_agent`.  Each slice runs on the WHOLE observation and state and keeps its own agent's rows, so
    agent a's rows (the state's too) are exactly `torch_forward_rnn`'s with slice a as the shared actor."""
    yc, hc = _rnn_step(critic, critic_rnn, xs, xo, xc, critic_state, is_init)
    value = F.linear(yc, critic["head_w"], critic["head_b"])
    if value_only:
        return RecurrentPolicyOutput(None, None, value, None, None, hc)
    E, A = xs.shape[:2]
    if eps is None and not deterministic:
        eps = torch.randn((E, A, ACTION_DIM), dtype=xs.dtype, device=xs.device, generator=generator)
    rows = []
    for a in range(A):
        p = agent_slice(actors, a)
        ya, ha = _rnn_step(p, agent_slice(actor_rnns, a), xs, xo, xc, actor_state, is_init)
        rows.append([t[:, a:a + 1] for t in (*_heads(p, ya, value, eps, deterministic, generator), ha)])
    action, log_prob, _, loc, ha = (torch.cat(t, dim=1) for t in zip(*rows))
    return RecurrentPolicyOutput(action, log_prob, value, loc, ha, hc)


def torch_act_rnn_per_agent(actors, actor_rnns, xs, xo, xc, state=None, is_init=None):
    """The CPU restatement of hns_policy_act_rnn_agents: the actor half of `torch_forward_rnn_per_agent` alone -> (loc [E, A, 4], the actors'
    states after the step [E, A, 128]); the same statements on the same operands, so the same bits as its deterministic action and state."""
    rows = []
    for a in range(xs.shape[1]):
        p = agent_slice(actors, a)
        ya, ha = _rnn_step(p, agent_slice(actor_rnns, a), xs, xo, xc, state, is_init)
        rows.append((F.linear(ya, p["head_w"], p["head_b"])[:, a:a + 1], ha[:, a:a + 1]))
    return tuple(torch.cat(t, dim=1) for t in zip(*rows))


class PerAgentRecurrentDevicePolicy(RecurrentDevicePolicy):
    """MAPPOPolicy with share_actor: False AND actor.rnn / critic.rnn — one actor and one actor GRU per pursuer, the critic and its GRU
    shared — in one HIP launch per call (`hns_policy_forward_rnn_agents`; `act_step`: `hns_policy_act_rnn_agents`).

    `PerAgentRecurrentDevicePolicy(actor_params, critic)`: actor_params the STACKED actor with its `rnn.*` leaves stacked too (every leaf
    [A, ...], as the reference's `actor_params` of this configuration), critic as for RecurrentDevicePolicy.  `from_checkpoint`, `refresh`,
    `forward`, `act_step`, `__call__` and `value` are RecurrentDevicePolicy's over the agents' entries: a tile is 32 envs of one agent and
    reads that agent's two images, the states stay [E, A, 128], and row (e, a) is bit for bit RecurrentDevicePolicy's with agent a's slices
    as the shared actor.  `scale` is [A, 4].  Refused with PolicyConfigError before anything is built: whatever RecurrentDevicePolicy
    refuses except share_actor: False; share_actor: True; tensors that are not stacked or whose leading sizes disagree; an rnn on only one
    of the two networks; a critic with stacked tensors; an observation with another number of agents (ValueError).  It is not trained on
    the device yet: every learner refuses it (DESIGN-open-items.md #13)."""
    per_agent = True
    _PACK, _FORWARD, _ACT = PerAgentDevicePolicy._PACK, PerAgentDevicePolicy._FORWARD, PerAgentDevicePolicy._ACT
    _FORWARD_RNN, _ACT_RNN = "hns_policy_forward_rnn_agents", "hns_policy_act_rnn_agents"

    def __init__(self, actor_params, critic, cfg=None, device=None, seed=0, agent_name="drone"):
        check_config_per_agent(cfg_without(cfg, "actor.rnn", "critic.rnn"))
        if is_stacked(critic, "base.attn.in_proj_weight"):
            raise PolicyConfigError("critic: parameters with a leading agent dimension; the reference stacks the actor only")
        actor_rest, self.actor_rnn, rnn_agents = split_rnn_per_agent(actor_params, "actor")
        critic_rest, self.critic_rnn = split_rnn(critic, "critic")
        actor_p, self.num_agents = parse_parameters_per_agent(actor_rest, "actor")
        if rnn_agents != self.num_agents:
            raise PolicyConfigError(f"actor: {self.num_agents} stacked actors with {rnn_agents} stacked GRUs")
        self._setup(actor_p, parse_parameters(critic_rest, CRITIC_NAMES, "critic"), device, seed, agent_name)
        self._setup_rnn()

    _packed_bytes, _pack_agents, scale = PerAgentDevicePolicy._packed_bytes, PerAgentDevicePolicy._pack_agents, PerAgentDevicePolicy.scale

    def _rnn_packed_bytes(self):
        return self._lib.hns_policy_rnn_packed_agents_bytes(self.num_agents)

    def _rnn_pack(self, a, c, st):
        return (self._lib.hns_policy_rnn_pack_agents(C.byref(a), C.byref(c), self.num_agents, self.rnn_packed.data_ptr(), st),
                "hns_policy_rnn_pack_agents")

    def _cpu_forward_rnn(self, *args):
        return torch_forward_rnn_per_agent(self.actor_p, self.critic_p, self.actor_rnn, self.critic_rnn, *args)

    def _cpu_act_rnn(self, *args):
        return torch_act_rnn_per_agent(self.actor_p, self.actor_rnn, *args)

    def _validate(self, xs, xo, xc):
        xs, xo, xc = super()._validate(xs, xo, xc)
        if xs.shape[1] != self.num_agents:
            raise ValueError(f"the observation has {xs.shape[1]} agents, the policy {self.num_agents} actors")
        return xs, xo, xc


def random_rnn_parameters_per_agent(num_agents, seed=0):
    """`random_rnn_parameters` for share_actor: False: `num_agents` independently initialised GRU blocks, every tensor [A, ...], under the
    reference's names with the `rnn.` prefix: merge it into `random_parameters_per_agent`'s stacked actor."""
    nets = [random_rnn_parameters(seed + 1000 * a) for a in range(num_agents)]
    return {k: torch.stack([n[k] for n in nets]).contiguous() for k in nets[0]}


def _td_get(td, key):
    try:
        return td.get(key, None) if hasattr(td, "get") else td[key]
    except KeyError:
        return None


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
