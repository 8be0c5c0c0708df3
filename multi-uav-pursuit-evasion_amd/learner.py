"""The MAPPO learner on the device: MAPPOPolicy.train_op (learning/mappo.py:363-475) over the update paths of this package.

`DeviceLearner(actor, critic, cfg, tp_net, value_normalizer)` holds what the reference's policy object holds for training — the two Adam
optimisers as `ClippedAdam`s, the predictor's `TPAdam(lr=1e-4)` (mappo.py:94), the ValueNorm1 instance, a `DevicePolicy` for the bootstrap
value — and `train_op(tensordict)` drives the five blocks in the reference's order:

    next_value  DevicePolicy.forward(value_only=True) on the last step's next observation          mappo.py:365-367, §7.3
    targets     gae.rollout_targets: denormalise, GAE, the moments, ValueNorm1, both normalisations  mappo.py:369-402, §7.1
    predictor   tp_train.update_tp over TP_epochs                                                    mappo.py:407-443, §7.2
    PPO loop    per epoch ONE randperm (tp_train.minibatches: make_dataset_naive's), per minibatch   mappo.py:446-461
                actor_train.update_actor, then critic_train.update_critic, both through index=       §7.5, §7.4
    info row    hns_learner_info: the column means of the per-minibatch table and action_norm         mappo.py:463-472

One RNG stream serves the call (the predictor's epochs draw first): `generator` goes to every randperm.  On the device the loop makes no host
synchronisation (the updates write their scalars into the rows of one table; no `.item()`, no index check); update_tp's selected-count read
stays, and the finished info row crosses to the host in one copy.  The two update workspaces and the info workspace are allocated once per
shape and reused by all ppo_epochs x num_minibatches calls.  CPU tensors run the same driver over the modules' CPU paths (CPU tests, gloo
runs — not the hot path).  DESIGN.md §7.6.

`RecurrentDeviceLearner` is the same driver for the `actor.rnn` / `critic.rnn` configuration: the bootstrap value from the stored
last critic state, the PPO loop over (env, segment) pairs through rnn_train.update_actor_rnn / update_critic_rnn.  `DeviceLearner` itself keeps
refusing a recurrent policy.

`PerAgentDeviceLearner` is the same for share_actor: False (one actor per agent): the actor block through
actor_train.update_actor_per_agent over the stacked tensors, everything else DeviceLearner's.  `DeviceLearner` keeps refusing that configuration.

`PerAgentRecurrentDeviceLearner` is `RecurrentDeviceLearner` for share_actor: False with actor.rnn / critic.rnn (one actor and one actor GRU per
agent): the actor step through rnn_train.update_actor_rnn_per_agent over the stacked tensors, everything else inherited.

`CentralCriticDeviceLearner` is the same for critic_input: state (the centralised critic): the critic block through
critic_train.update_critic_central on the stored state_drones, the bootstrap value from the last state, everything else DeviceLearner's.
`DeviceLearner` keeps refusing that configuration.

`PerAgentCentralCriticDeviceLearner` joins the two (share_actor: False with critic_input: state): the actor block is
PerAgentDeviceLearner's and the critic block, the rollout's state and the bootstrap value are CentralCriticDeviceLearner's — both classes are its
bases, so their method bodies are the ones that run.

`DeviceLearner._ppo_loop` is the only PPO loop.  A variant overrides what differs and nothing else: the units a permutation draws from
(`_units`), its update call for one index (`_actor_step`, `_critic_step`), its cached buffers (`_workspaces`), and its optimisers and tensors
(`_make_actor_opt`, `_make_critic_opt`, `_network_tensors`: checkpoints, buckets and the broadcast are written once over them).

`DeviceLearner(..., group=)` is the data-parallel learner: W ranks, each with the rollout of its own env slice, perform ONE
PPO update per minibatch on the union of their minibatches — the critic's branch decided on the union's sums, every mean over the union's
rows, the norm taken from the summed gradient, the predictor's ranks weighted by their selected windows.
`DataParallelRecurrentLearner` is the same for the recurrent configuration: `RecurrentDeviceLearner` over a process group,
through rnn_train's global forms (hns_rnn_actor_head_grad_global; hns_rnn_critic_head_sums, hns_rnn_critic_head_grad_global).
`DataParallelPerAgentLearner` and `DataParallelPerAgentRecurrentLearner` are the two per-agent learners over a process group (DESIGN.md
§7.19): the actor step through actor_train.update_actor_per_agent_global / rnn_train.update_actor_rnn_per_agent_global, the bucket and the
broadcast over the stacked tensors, everything else as the two data-parallel learners above."""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import abi, actor_train, critic_train, gae, rnn_train, sharding, tp_train
from . import policy as P
from . import policy_train as PT

ACTOR_COLUMNS = ("policy_loss", "entropy", "ESS", "actor_grad_norm")           # hns_actor_train_grad's four scalars, in its order
CRITIC_COLUMNS = ("value_loss", "explained_var", "critic_grad_norm")           # hns_critic_train_grad's three
COLUMNS = ACTOR_COLUMNS + CRITIC_COLUMNS
# train_info's keys in the reference's order of insertion (mappo.py:319-324, :348-352, :463-472)
INFO_KEYS = ("policy_loss", "actor_grad_norm", "entropy", "ESS", "value_loss", "critic_grad_norm", "explained_var", "TP_loss", "advantages_mean",
             "advantages_std", "action_norm", "value_running_mean")


class ValueNorm1(nn.Module):
    """The state of the reference's ValueNorm1 (learning/utils/valuenorm.py:41-103) under its buffer names, for a learner built without the
    reference's package: gae.rollout_targets updates it and reads `running_mean_var()`; its state_dict is the reference's."""

    def __init__(self, input_shape=(1,), beta=0.995, epsilon=1e-5):
        super().__init__()
        self.beta, self.epsilon = beta, epsilon
        self.register_buffer("running_mean", torch.zeros(input_shape))
        self.register_buffer("running_mean_sq", torch.zeros(input_shape))
        self.register_buffer("debiasing_term", torch.tensor(0.0))

    def running_mean_var(self):
        d = self.debiasing_term.clamp(min=self.epsilon)
        mean, mean_sq = self.running_mean / d, self.running_mean_sq / d
        return mean, (mean_sq - mean ** 2).clamp(min=1e-2)


def check_learner_config(cfg):
    """Every configuration actor_train.actor_cfg and critic_train.critic_cfg refuse (policy.check_config's among them), with their exception
    types, before anything is built."""
    actor_train.actor_cfg(cfg)
    critic_train.critic_cfg(cfg)


def _named(obj):
    """name -> tensor of a network (module, TensorDict-like or mapping) under the reference's names, `module.` prefixes dropped."""
    return {P._strip(k): v for k, v in P._flatten(obj).items()}


def _mean_row(table):
    """The CPU path's column means: hns_learner_info's statement (the fp64 sum in row order, divided once, rounded once to fp32)."""
    out = []
    for c in range(table.shape[1]):
        s = 0.0
        for v in table[:, c].tolist():
            s += v
        out.append(float(np.float32(s / table.shape[0])))
    return out


class DeviceLearner:
    """MAPPOPolicy's training half.  actor: the shared actor's parameters (TensorDictParams / TensorDict / mapping / nn.Module), critic: the
    critic module or its parameters — live tensors, updated in place; cfg: the algo cfg (dict or attribute object); tp_net: the predictor
    (tp_net.TPNet or the reference's TP_net) or None; value_normalizer: a ValueNorm1 (the reference's or this module's) or None; generator:
    the torch.Generator of every randperm (None: the global one); device_policy: a DevicePolicy over the same tensors (built when None).

    group: None — one process, the path above exactly — or a torch.distributed process group ("world": the default one): the ranks of the
    group train ONE set of networks from the rollouts of their env slices.  At construction and after load_state_dict the group's rank 0
    broadcasts the actor, the critic, the predictor, ValueNorm1's buffers and the three Adam states.  Per train_rollout one gather carries
    every rank's (num_minibatches, ppo_epochs, TP_epochs, predictor on, env-steps, agents): the settings must agree and every rank needs at
    least one env-step per minibatch, else ValueError on every rank before any further collective; global_rows per minibatch follows from
    it.  Each rank draws its own permutations of its own env-steps from its own `generator`.  Per minibatch: the actor's
    hns_actor_train_grad_global, SUM all-reduce of its bucket, hns_grad_norm, the step; the critic's hns_critic_train_sums, SUM all-reduce of
    five fp64 values, hns_critic_train_grad_global, SUM all-reduce of its bucket, hns_grad_norm, the step — three collectives per minibatch
    pair.  rollout_targets' gather is the existing one; the host adds no synchronisation of its own (gloo moves
    host copies: a correctness backend).
    Info row: every entry is the same on all ranks (one more all-reduce of three values per call).  value_loss, explained_var, entropy, the two gradient norms and the rollout moments are
    the union's by construction; policy_loss is the SUM of the ranks' shares (the union's loss); ESS is the MEAN of the ranks' own values —
    an approximation of a diagnostic (the effective sample size of the union is not the mean of the parts'), not used by the update;
    action_norm is the mean over all ranks' rows."""

    def __init__(self, actor, critic, cfg, tp_net=None, value_normalizer=None, agent_name="drone", generator=None, device_policy=None, group=None):
        check_learner_config(cfg)
        if getattr(device_policy, "recurrent", False):
            raise P.PolicyConfigError("DeviceLearner updates the non-recurrent networks only: a recurrent policy (actor.rnn / critic.rnn) is trained "
                                      "in torch over encoder.encode -> rnn.gru -> head (examples/recurrent_policy.py)")
        if getattr(device_policy, "central", False):
            raise P.PolicyConfigError("DeviceLearner updates the critic on the observation: a centralised critic (critic_input: state) is "
                                      "CentralCriticDeviceLearner's")
        self._configure(actor, critic, cfg, tp_net, value_normalizer, agent_name, generator)
        self._make_networks_state(device_policy, P.DevicePolicy)
        self._join(group)

    def _configure(self, actor, critic, cfg, tp_net, value_normalizer, agent_name, generator):
        """What every learner holds whatever its networks: the objects, train_op's settings from the algo cfg, the predictor's optimiser, the
        workspace cache.  The two networks' optimisers and the policy (_make_networks_state) and the group (_join) follow it."""
        get = PT.getter(cfg)
        self.cfg, self.agent_name, self.generator = cfg, agent_name, generator
        self.actor, self.critic, self.tp_net, self.value_normalizer = actor, critic, tp_net, value_normalizer
        self.ppo_epochs, self.tp_epochs = int(get("ppo_epochs", 4)), int(get("TP_epochs", 1))
        self.num_minibatches = int(get("num_minibatches", 16))
        self.normalize_advantages = bool(get("normalize_advantages", True))
        self.gamma, self.gae_lambda = float(get("gamma", 0.995)), float(get("gae_lambda", 0.95))
        self.use_tp = tp_net is not None and bool(get("use_TP_net", 1))
        if self.ppo_epochs < 1 or self.num_minibatches < 1 or (self.use_tp and self.tp_epochs < 1):
            raise ValueError("ppo_epochs, num_minibatches and TP_epochs must be >= 1")
        self.tp_opt = self._make_tp_opt() if tp_net is not None else None
        self.n_updates = 0
        self._ws = {}
        self.group = None
        self.actor_bucket = self.critic_bucket = self.tp_bucket = None

    # ---- a variant's two networks: their optimisers, their tensors in the optimisers' order
    def _make_actor_opt(self):
        return actor_train.make_optimizer(self.actor, self.cfg)

    def _make_critic_opt(self):
        return critic_train.make_optimizer(self.critic, self.cfg)

    def _network_tensors(self):
        """(the actor's tensors, the critic's): the order of a network's gradient bucket and of the broadcast."""
        return list(actor_train.actor_parameters(self.actor).values()), list(critic_train.critic_parameters(self.critic).values())

    def _make_tp_opt(self):
        return tp_train.TPAdam(tp_train.parameters(self.tp_net), lr=1e-4)

    def _make_networks_state(self, device_policy, policy_class):
        """The two networks' optimisers (the refusals of the cfg and of the parameters come first) and the policy of the bootstrap value."""
        self.actor_opt, self.critic_opt = self._make_actor_opt(), self._make_critic_opt()
        self.policy = device_policy if device_policy is not None else policy_class(self.actor, self.critic, self.cfg, agent_name=self.agent_name)

    def _optimizer_makers(self):
        """(attribute, state_dict key, maker) of the three optimisers."""
        return (("actor_opt", "actor_opt", self._make_actor_opt), ("critic_opt", "critic_opt", self._make_critic_opt), ("tp_opt", "TP_opt", self._make_tp_opt))

    def _make_network_buckets(self):
        """ONE flat gradient buffer per network, behind its tensors' .grad."""
        self.actor_bucket, self.critic_bucket = (PT.GradBucket(t) for t in self._network_tensors())

    # ---- the data-parallel path's state
    def _join(self, group):
        """The data-parallel learner's part of construction: the group, the gradient buckets, rank 0's state on every rank."""
        self.group = sharding.resolve_group(group)
        if self.group is not None:
            self.world = torch.distributed.get_world_size(self.group)
            self._make_network_buckets()
            self.tp_bucket = PT.GradBucket(tp_train.parameters(self.tp_net)) if self.tp_net is not None else None
            self._broadcast_state()

    def _broadcast_state(self):
        """Rank 0 of the group hands every rank its networks, ValueNorm1 buffers and Adam states (tensor by tensor: construction and checkpoint
        loading only)."""
        dist = torch.distributed
        tensors = [t for net in self._network_tensors() for t in net]
        if self.tp_net is not None:
            tensors += tp_train.parameters(self.tp_net)
        if self.value_normalizer is not None:
            tensors += [getattr(self.value_normalizer, k) for k in ("running_mean", "running_mean_sq", "debiasing_term")]
        for t in tensors:
            sharding.broadcast_from_first(t, self.group)
        first = dist.get_rank(self.group) == 0
        to_cpu = lambda o: (o.detach().cpu() if torch.is_tensor(o) else {k: to_cpu(v) for k, v in o.items()} if isinstance(o, dict) else   # noqa: E731
                            [to_cpu(v) for v in o] if isinstance(o, list) else o)
        box = [{name: to_cpu(getattr(self, name).state_dict()) for name, _, _ in self._optimizer_makers() if getattr(self, name) is not None} if first else None]
        dist.broadcast_object_list(box, src=dist.get_global_rank(self.group, 0), group=self.group)
        if not first:
            for name, _, make in self._optimizer_makers():
                if getattr(self, name) is None:
                    continue
                setattr(self, name, make())
                if box[0][name]["state"]:
                    getattr(self, name).load_state_dict(box[0][name])

    def _global_counts(self, steps, agents, unit="env-steps", rows_per_unit=1, more=()):
        """The rollout's one gather of settings and counts -> (rows of a minibatch over all ranks, rows of the rollout over all ranks).  Every
        rank sees the same table, so a refusal is raised by all of them, before any collective whose shape or count depends on what
        disagrees.  `steps`: what this rank's permutation draws from — env-steps, or a recurrent learner's `unit` of `rows_per_unit` steps
        each; `more`: further (name, value) settings that must agree."""
        table = sharding.all_gather_rows([self.num_minibatches, self.ppo_epochs, self.tp_epochs if self.use_tp else 0, int(self.use_tp), steps, agents,
                                          *(v for _, v in more)], self.group)
        for c, what in ((0, "num_minibatches"), (1, "ppo_epochs"), (2, "TP_epochs"), (3, "use_TP_net"), (5, "the number of agents"),
                        *((6 + i, name) for i, (name, _) in enumerate(more))):
            if len(set(table[:, c].tolist())) != 1:
                raise ValueError(f"{what} differs across the ranks of the group: {table[:, c].tolist()}")
        short = [r for r, n in enumerate(table[:, 4].tolist()) if n < self.num_minibatches]
        if short:
            raise ValueError(f"ranks {short} hold fewer {unit} than num_minibatches {self.num_minibatches}: {table[:, 4].tolist()}")
        return (sum(n // self.num_minibatches for n in table[:, 4].tolist()) * rows_per_unit * agents,
                sum(table[:, 4].tolist()) * rows_per_unit * agents)

    def _reduce_info(self, head, rows, total_rows):
        """The three entries of [column means, action_norm] that differ from rank to rank, in ONE all-reduce of three fp64 values: policy_loss
        becomes the sum of the ranks' shares, ESS the mean of the ranks' values, action_norm the mean over all ranks' rows (each rank's mean
        times its row count, exact in fp64, over the total).  With one rank every value keeps its bits."""
        cols = [COLUMNS.index("policy_loss"), COLUMNS.index("ESS"), len(COLUMNS)]
        v = head[cols].double()
        v[2] *= rows
        sharding.all_reduce_sum(v, self.group)
        head = head.clone()
        head[cols[0]], head[cols[1]], head[cols[2]] = v[0].float(), (v[1] / self.world).float(), (v[2] / total_rows).float()
        return head

    # ---- workspaces
    def _workspace(self, name, nbytes, device):
        """The cached buffer of `name`, reallocated only when the shape grows (or the device changes)."""
        ws = self._ws.get(name)
        if ws is None or ws.numel() < nbytes or ws.device != device:
            ws = self._ws[name] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return ws

    def release(self):
        """Drop the cached workspaces (the next train_op allocates them again)."""
        self._ws = {}

    # ---- the reference's entry point
    def train_op(self, tensordict):
        """MAPPOPolicy.train_op on the collector's [N, T] tensordict; returns {"<agent>/policy_loss": float, ...}."""
        return self.train_rollout(**self._rollout_kwargs(tensordict))

    def _rollout_kwargs(self, td):
        """train_rollout's keyword arguments from the reference's tensordict keys."""
        obs = td[("agents", "observation")]
        nxt = td["next"]
        last = nxt[("agents", "observation")]
        pick = lambda o, k: o.get(k, None) if hasattr(o, "get") else o[k]          # noqa: E731
        agent_done = nxt.get(f"{self.agent_name}.done", None) if hasattr(nxt, "get") else None
        tp = None
        if self.use_tp:
            t = nxt[("agents", "TP")]
            tp = (t["TP_input"], t["TP_groundtruth"], t["TP_done"])
        xo_last = pick(last, "state_others")
        return dict(
            obs_self=obs["state_self"], obs_others=pick(obs, "state_others"), obs_cylinders=obs["cylinders"], action=td[("agents", "action")],
            log_probs=td[f"{self.agent_name}.action_logp"], state_value=td["state_value"],
            next_obs_last=(last["state_self"][:, -1], xo_last[:, -1] if xo_last is not None else None, last["cylinders"][:, -1]),
            reward=nxt[("agents", "reward")], done=nxt["done"], agent_done=agent_done, tp=tp)

    def train_rollout(self, *, obs_self, obs_others, obs_cylinders, action, log_probs, state_value, next_obs_last, reward, done, agent_done=None,
                      tp=None):
        """train_op on tensors: observations [N, T, A, ...], action [N, T, A, 4], log_probs / state_value [N, T, A, 1], next_obs_last: the
        (state_self, state_others, cylinders) of the last step's next observation [N, A, ...], reward [N, T, A, r], done [N, T, 1] (the env's),
        agent_done [N, T, A, 1] or None, tp: (TP_input, TP_groundtruth, TP_done) with the predictor."""
        return self._run(None, obs_self, obs_others, obs_cylinders, action, log_probs, state_value, next_obs_last, reward, done, agent_done, tp)

    def _run(self, recurrent, obs_self, obs_others, obs_cylinders, action, log_probs, state_value, next_obs_last, reward, done, agent_done, tp):
        """train_rollout's blocks.  `recurrent`: None, or what a recurrent learner's two hooks (_bootstrap_value, _ppo_loop) need beside the
        rollout — handed down to them untouched."""
        if self.use_tp and tp is None:
            raise ValueError("use_TP_net: the rollout's TP_input, TP_groundtruth and TP_done are needed (tp=)")
        xs, xo, xc = PT.as_rollout(obs_self, obs_others, obs_cylinders)
        N, T, A, _ = xs.shape
        dev = xs.device
        global_rows, total_rows = self._rollout_counts(N, T, A) if self.group is not None else (None, None)
        # mappo.py:354-361: done = agent_done | env_done (an absent agent_done is env_done, which rollout_targets broadcasts over the agents)
        dones = done.unsqueeze(-1)
        if agent_done is not None:
            dones = agent_done | dones
        with torch.no_grad():
            next_value = self._bootstrap_value(next_obs_last, recurrent)
        adv, ret, _, (adv_mean, adv_std) = gae.rollout_targets(reward, dones, state_value, next_value, self.gamma, self.gae_lambda,
                                                               value_normalizer=self.value_normalizer, normalize_advantages=self.normalize_advantages,
                                                               return_moments=True)
        tp_loss = None
        if self.use_tp:
            tp_loss = tp_train.update_tp(self.tp_net, *tp, self.tp_net.future_predcition_step, self.tp_net.window_step, self.num_minibatches,
                                         self.tp_epochs, self.tp_opt, generator=self.generator,
                                         **(dict(group=self.group, bucket=self.tp_bucket) if self.group is not None else {}))
        M = self.ppo_epochs * self.num_minibatches
        table = torch.empty(M, len(COLUMNS), dtype=torch.float32, device=dev)
        self._ppo_loop(xs, xo, xc, action, log_probs, adv, state_value, ret, table, global_rows, recurrent)
        extras = [t.reshape(()).to(torch.float32) for t in ([tp_loss] if self.use_tp else []) + [adv_mean, adv_std]]
        if self.value_normalizer is not None:
            extras.append(self.value_normalizer.running_mean.mean().to(torch.float32))
        if dev.type == "cuda":
            head = self._info_row(action, table)
        else:
            a = action.reshape(-1, action.shape[-1]).double()
            norm = float(np.float32(a.square().sum(-1).sqrt().sum().item() / a.shape[0]))
            head = torch.tensor(_mean_row(table) + [norm], dtype=torch.float32)
        if self.group is not None:
            head = self._reduce_info(head, N * T * A, total_rows)
        if dev.type == "cuda":
            row = torch.cat([head, torch.stack(extras)]).tolist()                                   # the call's one copy to the host
        else:
            row = head.tolist() + [float(t) for t in extras]
        info = dict(zip(COLUMNS + ("action_norm",), row))
        rest = iter(row[len(COLUMNS) + 1:])
        if self.use_tp:
            info["TP_loss"] = next(rest)
        info["advantages_mean"], info["advantages_std"] = next(rest), next(rest)
        if self.value_normalizer is not None:
            info["value_running_mean"] = next(rest)
        self.n_updates += 1
        return {f"{self.agent_name}/{k}": info[k] for k in INFO_KEYS if k in info}

    def _rollout_counts(self, N, T, A):
        """The data-parallel path's (rows of a minibatch, rows of the rollout) over all ranks."""
        return self._global_counts(N * T, A)

    def _bootstrap_value(self, next_obs_last, recurrent=None):
        """mappo.py:365-367: the critic's value of the last step's next observation, ONE value_only call."""
        return self.policy.forward(*next_obs_last, value_only=True).value

    # ---- the PPO loop and what a variant supplies to it
    def _units(self, N, T):
        """What a permutation draws from: the rollout's env-steps."""
        return N * T

    def _workspaces(self, xs, xc, actor_workspace_bytes=None):
        """The device loop's (actor, critic) workspaces, cached between calls.  actor_workspace_bytes: the actor entry's query (None:
        hns_actor_train_workspace_bytes)."""
        N, T, A, D = xs.shape
        dev, K, lib = xs.device, int(xc.shape[3]), abi.load_library()
        rows = (N * T // self.num_minibatches) * A
        na, nc = (actor_workspace_bytes or lib.hns_actor_train_workspace_bytes)(rows, D, A, K), lib.hns_critic_train_workspace_bytes(rows, D, A, K)
        if rows < 1 or na == 0 or nc == 0:
            raise ValueError(f"shape outside the kernels' limits: {rows} rows per minibatch, self_dim {D}, {A} agents, {K} cylinders")
        return self._workspace("actor", na, dev), self._workspace("critic", nc, dev)

    def _actor_step(self, idx, obs, action, log_probs, adv, recurrent, **kw):
        return actor_train.update_actor(self.actor, *obs, action, log_probs, adv, self.actor_opt, index=idx, cfg=self.cfg, **kw)

    def _critic_step(self, idx, obs, state_value, ret, recurrent, **kw):
        return critic_train.update_critic(self.critic, *obs, state_value, ret, self.critic_opt, index=idx, cfg=self.cfg, **kw)

    def _ppo_loop(self, xs, xo, xc, action, log_probs, adv, state_value, ret, table, global_rows=None, recurrent=None):
        """mappo.py:446-461: per epoch one permutation of the variant's units, per minibatch the actor's update and then the critic's.  On
        the device: no host synchronisation — cached workspaces, scalars written into `table`'s rows, no index check.  `global_rows` (the
        data-parallel path): the updates' global forms over the group.  Each network's gradients lie in its bucket where the learner holds
        one."""
        N, T = xs.shape[:2]
        dev, obs, na = xs.device, (xs, xo, xc), len(ACTOR_COLUMNS)
        ws_a, ws_c = self._workspaces(xs, xc) if dev.type == "cuda" else (None, None)
        kw_a, kw_c = {"bucket": self.actor_bucket}, {"bucket": self.critic_bucket}
        if global_rows is not None:
            kw_a.update(global_rows=global_rows, entropy_share=1.0 / self.world, group=self.group)
            kw_c.update(global_rows=global_rows, group=self.group)
        m = 0
        for _ in range(self.ppo_epochs):
            for idx in tp_train.minibatches(self._units(N, T), self.num_minibatches, dev, self.generator):
                out_a, out_c = (table[m, :na], table[m, na:]) if ws_a is not None else (None, None)
                sa = self._actor_step(idx, obs, action, log_probs, adv, recurrent, workspace=ws_a, out=out_a, **kw_a)
                sc = self._critic_step(idx, obs, state_value, ret, recurrent, workspace=ws_c, out=out_c, **kw_c)
                if ws_a is None:                                 # CPU: the updates return their scalars
                    table[m] = torch.stack([(sa | sc)[k].reshape(()).to(torch.float32) for k in COLUMNS])
                m += 1

    def _info_row(self, action, table):
        """hns_learner_info: [column means, action_norm] as a device tensor (two launches, no synchronisation)."""
        a = action.reshape(-1, action.shape[-1])
        if a.dtype != torch.float32:
            raise TypeError(f"action must be float32, not {a.dtype}")
        dev, lib = a.device, abi.load_library()
        nbytes = lib.hns_learner_info_workspace_bytes(a.shape[0])
        ws = self._workspace("info", nbytes, dev)
        out = torch.empty(table.shape[1] + 1, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.hns_learner_info(a.data_ptr(), (C.c_int64 * 2)(a.stride(0), a.stride(1)), a.shape[0], a.shape[1], table.data_ptr(),
                                      table.shape[0], table.shape[1], out.data_ptr(), ws.data_ptr(), ws.numel(),
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        abi.check(rc, "hns_learner_info")
        return out

    # ---- checkpoints
    def state_dict(self):
        """MAPPOPolicy.state_dict()'s entries (mappo.py:477-484: "TP", "critic", "actor_params", "value_normalizer"; an absent part is left
        out) and the three optimisers in torch.optim.Adam's format ("actor_opt", "critic_opt", "TP_opt"), which the reference drops."""
        sd = {}
        if self.tp_net is not None:
            sd["TP"] = self.tp_net.state_dict()
        sd["critic"] = self.critic.state_dict() if isinstance(self.critic, nn.Module) else {k: v.detach() for k, v in P._flatten(self.critic).items()}
        sd["actor_params"] = self.actor if hasattr(self.actor, "flatten_keys") else {k: v.detach() for k, v in P._flatten(self.actor).items()}
        if self.value_normalizer is not None:
            sd["value_normalizer"] = self.value_normalizer.state_dict() if hasattr(self.value_normalizer, "state_dict") else \
                {k: getattr(self.value_normalizer, k) for k in ("running_mean", "running_mean_sq", "debiasing_term")}
        sd["actor_opt"], sd["critic_opt"] = self.actor_opt.state_dict(), self.critic_opt.state_dict()
        if self.tp_opt is not None:
            sd["TP_opt"] = self.tp_opt.state_dict()
        return sd

    def load_state_dict(self, sd):
        """A checkpoint of state_dict() or of the reference (no optimiser keys: fresh optimisers, as mappo.py:486-491 leaves them).  Every
        tensor is copied into the live parameter, so its version counter moves and DevicePolicy and the env's predictor re-pack."""
        with torch.no_grad():
            for mine, theirs, what in ((self.actor, sd["actor_params"], "actor_params"), (self.critic, sd["critic"], "critic")):
                dst, src = _named(mine), _named(theirs)
                if set(dst) != set(src):
                    raise KeyError(f"{what}: parameter names differ: {sorted(set(dst) ^ set(src))[:6]}")
                for k, v in dst.items():
                    v.copy_(src[k])
            if self.tp_net is not None and "TP" in sd:
                self.tp_net.load_state_dict(sd["TP"])
            if self.value_normalizer is not None and "value_normalizer" in sd:
                if hasattr(self.value_normalizer, "load_state_dict"):
                    self.value_normalizer.load_state_dict(sd["value_normalizer"])
                else:
                    for k, v in sd["value_normalizer"].items():
                        getattr(self.value_normalizer, k).copy_(v)
        for name, key, make in self._optimizer_makers():
            if getattr(self, name) is None:
                continue
            setattr(self, name, make())
            if key in sd:
                getattr(self, name).load_state_dict(sd[key])
        if self.group is not None:                               # one state on every rank: rank 0's
            self._broadcast_state()


class PerAgentDeviceLearner(DeviceLearner):
    """MAPPOPolicy's training half with share_actor: False (one actor per agent): `DeviceLearner`'s train_op / train_rollout,
    info row and state_dict, with the actor block through actor_train.update_actor_per_agent (one `hns_actor_train_grad_agents` call and one
    ClippedAdam step over the 23 stacked tensors per minibatch, a cached workspace, no host synchronisation in the PPO loop).  The critic
    block, the targets, the predictor and the bootstrap value are DeviceLearner's, unchanged.

    actor: the STACKED actor's parameters (every tensor [A, ...]: the reference's actor_params; "actor_params" of state_dict()), live tensors
    updated in place; device_policy: a PerAgentDevicePolicy over the same tensors (built when None).  Refused before anything is built:
    group= (NotImplementedError: the data-parallel form is DataParallelPerAgentLearner), a recurrent policy and whatever PerAgentDevicePolicy
    refuses (PolicyConfigError), a device_policy that is not per-agent, and the cfg refusals of DeviceLearner with their exception types."""

    def __init__(self, actor, critic, cfg, tp_net=None, value_normalizer=None, agent_name="drone", generator=None, device_policy=None, group=None):
        if group is not None:
            raise NotImplementedError("PerAgentDeviceLearner takes no group=: data-parallel training of per-agent actors is "
                                      "DataParallelPerAgentLearner's")
        if getattr(device_policy, "recurrent", False):
            raise P.PolicyConfigError("PerAgentDeviceLearner updates the non-recurrent networks only: per-agent actors with actor.rnn / critic.rnn are "
                                      "not implemented")
        if device_policy is not None and not getattr(device_policy, "per_agent", False):
            raise P.PolicyConfigError("PerAgentDeviceLearner needs a PerAgentDevicePolicy (a shared actor is DeviceLearner's)")
        actor_train.actor_cfg_per_agent(cfg)
        shared = P.cfg_without(cfg, "share_actor")               # what the shared critic's functions (and policy.check_config behind them) take
        critic_train.critic_cfg(shared)
        self._configure(actor, critic, shared, tp_net, value_normalizer, agent_name, generator)
        self._make_networks_state(device_policy, P.PerAgentDevicePolicy)

    def _make_actor_opt(self):
        return actor_train.make_optimizer_per_agent(self.actor, self.cfg)

    def _network_tensors(self):
        """The 23 stacked tensors in the optimiser's order, and the shared critic's."""
        return list(actor_train.actor_parameters_per_agent(self.actor).values()), list(critic_train.critic_parameters(self.critic).values())

    def _workspaces(self, xs, xc):
        return super()._workspaces(xs, xc, abi.load_library().hns_actor_train_agents_workspace_bytes)

    def _actor_step(self, idx, obs, action, log_probs, adv, recurrent, bucket=None, **kw):        # (no group, so no bucket)
        return actor_train.update_actor_per_agent(self.actor, *obs, action, log_probs, adv, self.actor_opt, index=idx, cfg=self.cfg, **kw)


class CentralCriticDeviceLearner(DeviceLearner):
    """MAPPOPolicy's training half with critic_input: state (the centralised critic: ONE row per env over the state, v_out = Linear(128, A);
    DESIGN.md §7.20): `DeviceLearner`'s train_op / train_rollout, info row, state_dict and checkpoint (the reference's, with the central
    critic's names), with the critic block through critic_train.update_critic_central (one `hns_critic_train_grad_central` call and one
    ClippedAdam step over the critic's 20 tensors per minibatch, a cached workspace, no host synchronisation in the PPO loop) and the
    bootstrap value from the policy's value_only call on the last step's next state.  The actor block, the targets, the predictor and the
    info row are DeviceLearner's, unchanged.

    critic: the centralised critic's parameters (policy.CENTRAL_CRITIC_NAMES), live tensors updated in place; device_policy: a
    CentralCriticDevicePolicy over the same tensors (built when None).  train_rollout takes two more tensors: state_drones [N, T, A, D] and
    next_state_last [N, A, D] (RolloutStorage.learner_kwargs() of a collector over such a policy); the state's cylinders are agent 0's rows
    of obs_cylinders, read in place.  Refused before anything is built: group= (NotImplementedError: there is no data-parallel form), a
    recurrent or per-agent policy, a device_policy that is not a CentralCriticDevicePolicy, critic_input: obs, and whatever
    CentralCriticDevicePolicy and the cfg checks of DeviceLearner refuse, with their exception types."""

    def __init__(self, actor, critic, cfg, tp_net=None, value_normalizer=None, agent_name="drone", generator=None, device_policy=None, group=None):
        if group is not None:
            raise NotImplementedError("CentralCriticDeviceLearner takes no group=: the centralised critic has no data-parallel form")
        if getattr(device_policy, "recurrent", False) or getattr(device_policy, "per_agent", False):
            raise P.PolicyConfigError("CentralCriticDeviceLearner updates the shared non-recurrent actor and the centralised critic only")
        if device_policy is not None and not getattr(device_policy, "central", False):
            raise P.PolicyConfigError("CentralCriticDeviceLearner needs a CentralCriticDevicePolicy (a critic on the observation is DeviceLearner's)")
        P.check_config_central(cfg)
        rest = P.cfg_without(cfg, "critic_input")                # what the actor's functions (and policy.check_config behind them) take
        actor_train.actor_cfg(rest)
        critic_train.critic_cfg(rest, central=True)
        self._configure(actor, critic, rest, tp_net, value_normalizer, agent_name, generator)
        self._make_networks_state(device_policy, P.CentralCriticDevicePolicy)

    def _network_tensors(self):
        return list(actor_train.actor_parameters(self.actor).values()), list(critic_train.central_critic_parameters(self.critic).values())

    def _rollout_kwargs(self, td):
        """DeviceLearner's, and the state the critic reads: ("agents", "state", "state_drones") of every step and of the last step's next."""
        kw = super()._rollout_kwargs(td)
        kw["state_drones"] = td[("agents", "state")]["state_drones"]
        kw["next_state_last"] = td["next"][("agents", "state")]["state_drones"][:, -1]
        return kw

    def train_rollout(self, *, obs_self, obs_others, obs_cylinders, action, log_probs, state_value, next_obs_last, reward, done, agent_done=None,
                      tp=None, state_drones=None, next_state_last=None):
        """DeviceLearner.train_rollout's arguments and the critic's: state_drones [N, T, A, D], next_state_last [N, A, D]."""
        if state_drones is None or next_state_last is None:
            raise ValueError("a centralised critic's rollout needs state_drones and next_state_last (RolloutStorage.learner_kwargs())")
        if state_drones.dim() != 4 or tuple(state_drones.shape[:3]) != tuple(action.shape[:3]):
            raise ValueError(f"state_drones must be [N, T, A, D] over the rollout's {tuple(action.shape[:3])}, not {tuple(state_drones.shape)}")
        rk = dict(state_drones=state_drones, next_state_last=next_state_last)
        return self._run(rk, obs_self, obs_others, obs_cylinders, action, log_probs, state_value, next_obs_last, reward, done, agent_done, tp)

    def _bootstrap_value(self, next_obs_last, rk=None):
        return self.policy.forward(*next_obs_last, rk["next_state_last"], value_only=True).value

    def _workspaces(self, xs, xc):
        N, T, A, D = xs.shape
        dev, K, lib = xs.device, int(xc.shape[3]), abi.load_library()
        batch = N * T // self.num_minibatches
        na, nc = lib.hns_actor_train_workspace_bytes(batch * A, D, A, K), lib.hns_critic_train_central_workspace_bytes(batch, D, A, K)
        if batch < 1 or na == 0 or nc == 0:
            raise ValueError(f"shape outside the kernels' limits: {batch} env-steps per minibatch, self_dim {D}, {A} agents, {K} cylinders")
        return self._workspace("actor", na, dev), self._workspace("critic", nc, dev)

    def _critic_step(self, idx, obs, state_value, ret, rk, bucket=None, **kw):                      # (no group, so no bucket)
        return critic_train.update_critic_central(self.critic, rk["state_drones"], obs[2], state_value, ret, self.critic_opt, index=idx,
                                                  cfg=self.cfg, **kw)


class PerAgentCentralCriticDeviceLearner(PerAgentDeviceLearner, CentralCriticDeviceLearner):
    """MAPPOPolicy's training half with share_actor: False AND critic_input: state (one actor per agent under ONE centralised critic over the
    joint state): the join of its two bases, whose method bodies run unchanged.  PerAgentDeviceLearner's: the actor's
    optimiser and the actor step (actor_train.update_actor_per_agent over the 23 stacked tensors).  CentralCriticDeviceLearner's:
    `_rollout_kwargs`, `train_rollout(..., state_drones, next_state_last)`, the bootstrap value and the critic step
    (critic_train.update_critic_central over the critic's 20 tensors).  DeviceLearner's: train_op, the targets, the predictor, the info row,
    state_dict / load_state_dict and the checkpoint (the stacked "actor_params" beside the central critic's names).  Its own: the pairing of
    the two halves in `_network_tensors` and `_workspaces` (hns_actor_train_agents_workspace_bytes,
    hns_critic_train_central_workspace_bytes).

    actor: the STACKED actor's parameters; critic: the centralised critic's — live tensors, updated in place; device_policy: a
    PerAgentCentralCriticDevicePolicy over the same tensors (built when None).  Refused before anything is built: group=
    (NotImplementedError: there is no data-parallel form), a recurrent policy, a device_policy that is not both per-agent and central,
    share_actor: True, critic_input: obs, and whatever the two bases' cfg checks refuse, with their exception types."""

    def __init__(self, actor, critic, cfg, tp_net=None, value_normalizer=None, agent_name="drone", generator=None, device_policy=None, group=None):
        if group is not None:
            raise NotImplementedError("PerAgentCentralCriticDeviceLearner takes no group=: per-agent actors beside the centralised critic have no "
                                      "data-parallel form")
        if getattr(device_policy, "recurrent", False):
            raise P.PolicyConfigError("PerAgentCentralCriticDeviceLearner updates the non-recurrent networks only: the centralised critic with "
                                      "actor.rnn / critic.rnn is not implemented")
        if device_policy is not None and not (getattr(device_policy, "per_agent", False) and getattr(device_policy, "central", False)):
            raise P.PolicyConfigError("PerAgentCentralCriticDeviceLearner needs a PerAgentCentralCriticDevicePolicy (a shared actor beside the "
                                      "centralised critic is CentralCriticDeviceLearner's, per-agent actors beside the critic on the observation "
                                      "PerAgentDeviceLearner's)")
        P.check_config_per_agent_central(cfg)
        rest = P.cfg_without(cfg, "share_actor", "critic_input")     # what both halves' functions (and policy.check_config behind them) take
        actor_train.actor_cfg_per_agent(rest)
        critic_train.critic_cfg(rest, central=True)
        self._configure(actor, critic, rest, tp_net, value_normalizer, agent_name, generator)
        self._make_networks_state(device_policy, P.PerAgentCentralCriticDevicePolicy)

    def _network_tensors(self):
        """The 23 stacked tensors in the actor optimiser's order, and the centralised critic's 20."""
        return list(actor_train.actor_parameters_per_agent(self.actor).values()), list(critic_train.central_critic_parameters(self.critic).values())

    def _workspaces(self, xs, xc):
        N, T, A, D = xs.shape
        dev, K, lib = xs.device, int(xc.shape[3]), abi.load_library()
        batch = N * T // self.num_minibatches
        na, nc = lib.hns_actor_train_agents_workspace_bytes(batch * A, D, A, K), lib.hns_critic_train_central_workspace_bytes(batch, D, A, K)
        if batch < 1 or na == 0 or nc == 0:
            raise ValueError(f"shape outside the kernels' limits: {batch} env-steps per minibatch, self_dim {D}, {A} agents, {K} cylinders")
        return self._workspace("actor", na, dev), self._workspace("critic", nc, dev)


class RecurrentDeviceLearner(DeviceLearner):
    """MAPPOPolicy's training half with actor.rnn / critic.rnn: `DeviceLearner`'s blocks in its order, with the recurrent pieces in place.

    actor, critic: the networks' parameters under the reference's names with their `rnn.*` tensors (what RecurrentDevicePolicy parses) — live
    tensors, updated in place; cfg: the algo cfg (actor.rnn.train_seq_len: the segment length L, default 16); device_policy: a
    RecurrentDevicePolicy over the same tensors (built when None).  Two ClippedAdams, one per network as the reference holds them, each
    over the encoder's, the GRU's and the head's tensors; the predictor's TPAdam.

        next_value  ONE policy.forward(..., critic_state=last_critic_rnn_state, is_init=last_is_init, value_only=True)
        targets     gae.rollout_targets, exactly DeviceLearner's call
        predictor   tp_train.update_tp, unchanged (the reference groups the predictor's windows in runs of seq_len before it permutes them; the
                    loss is a mean over windows, so only which windows share a minibatch differs)
        PPO loop    per epoch ONE permutation of the N T / L segments (make_dataset_naive's randperm((N S // M) M).reshape(M, -1), the same
                    generator calls), per minibatch rnn_train.update_actor_rnn, then update_critic_rnn; on the device no host
                    synchronisation, the scalars land in the rows of the [M, 7] table, every buffer is kept per network between calls
        info row    hns_learner_info, INFO_KEYS, one copy to the host

    Refused: group= (data-parallel recurrent training is DataParallelRecurrentLearner's), the configurations RecurrentDevicePolicy refuses, a non-recurrent device_policy, a
    per_agent device_policy or stacked actor tensors (recurrent per-agent actors are PerAgentRecurrentDeviceLearner's: DESIGN.md §7.18), a
    rollout whose T train_seq_len does not divide (or whose storage was cut with another segment length)."""

    def __init__(self, actor, critic, cfg, tp_net=None, value_normalizer=None, generator=None, device_policy=None, agent_name="drone", group=None):
        if group is not None:
            raise NotImplementedError("RecurrentDeviceLearner takes no group=: data-parallel recurrent training is DataParallelRecurrentLearner's")
        if device_policy is not None and not getattr(device_policy, "recurrent", False):
            raise P.PolicyConfigError("RecurrentDeviceLearner needs a RecurrentDevicePolicy (a non-recurrent policy is DeviceLearner's)")
        if getattr(device_policy, "per_agent", False) or P.is_stacked(actor):
            raise P.PolicyConfigError(f"{type(self).__name__} updates ONE shared recurrent actor: recurrent per-agent actors (share_actor: False with "
                                      "actor.rnn) are PerAgentRecurrentDeviceLearner's, and data-parallel "
                                      "DataParallelPerAgentRecurrentLearner's, which closed the open item DESIGN-open-items.md #13")
        self._build(actor, critic, cfg, tp_net, value_normalizer, agent_name, generator, device_policy, P.RecurrentDevicePolicy)

    stacked_actor = False                                        # PerAgentRecurrentDeviceLearner: the actor's tensors are stacked over the agents

    def _build(self, actor, critic, cfg, tp_net, value_normalizer, agent_name, generator, device_policy, policy_class):
        """What follows the refusals of the constructor's own arguments: the settings, the segment length, the optimisers, the policy, the
        two networks' buffers."""
        self._configure(actor, critic, cfg, tp_net, value_normalizer, agent_name, generator)
        self.train_seq_len = rnn_train.train_seq_len(cfg)
        if not 1 <= self.train_seq_len <= abi.HNS_GRU_MAX_STEPS:
            raise ValueError(f"actor.rnn.train_seq_len must be in [1, {abi.HNS_GRU_MAX_STEPS}], not {self.train_seq_len}")
        self._make_networks_state(device_policy, policy_class)
        self._rnn_ws = (rnn_train.RnnWorkspace(), rnn_train.RnnWorkspace())

    def _make_actor_opt(self):
        return rnn_train.make_optimizer(self.actor, self.cfg, actor=True, stacked=self.stacked_actor)

    def _make_critic_opt(self):
        return rnn_train.make_optimizer(self.critic, self.cfg, actor=False)

    def _network_tensors(self):
        return tuple(rnn_train.flat_parameters(rnn_train.network_parameters(net, actor, actor and self.stacked_actor))
                     for net, actor in ((self.actor, True), (self.critic, False)))

    def release(self):
        super().release()
        for ws in self._rnn_ws:
            ws.release()

    def train_op(self, tensordict):
        """MAPPOPolicy.train_op on the collector's [N, T] tensordict with the reference's recurrent keys: "is_init" [N, T, 1] and
        "<agent>.actor_rnn_state" / "<agent>.critic_rnn_state" — the state going INTO every step [N, T, A, 128] (every train_seq_len-th
        step's is the segment's; a [N, T / L, A, 128] tensor is taken as it is) — and, under "next", the critic state and "is_init" (absent:
        "done") after the last step."""
        td, L = tensordict, self.train_seq_len
        nxt = td["next"]
        ka, kc = f"{self.agent_name}.actor_rnn_state", f"{self.agent_name}.critic_rnn_state"
        T = td["is_init"].shape[1]
        seg = lambda t: t if t.shape[1] * L == T and L > 1 else t[:, ::L].contiguous()          # noqa: E731
        nget = lambda k: nxt.get(k, None) if hasattr(nxt, "get") else nxt[k]                     # noqa: E731
        last_init = nget("is_init")
        return self.train_rollout(**self._rollout_kwargs(td), is_init=td["is_init"], actor_rnn_state=seg(td[ka]), critic_rnn_state=seg(td[kc]),
                                  rnn_seq_len=L, last_critic_rnn_state=nxt[kc][:, -1].contiguous(),
                                  last_is_init=(last_init if last_init is not None else nxt["done"])[:, -1])

    def train_rollout(self, *, obs_self, obs_others, obs_cylinders, action, log_probs, state_value, next_obs_last, reward, done, agent_done=None,
                      tp=None, is_init=None, actor_rnn_state=None, critic_rnn_state=None, rnn_seq_len=None, last_critic_rnn_state=None,
                      last_is_init=None):
        """train_op on tensors: RolloutStorage.learner_kwargs() (DeviceLearner.train_rollout's arguments) and recurrent_kwargs() — is_init
        [N, T, 1]; actor_rnn_state, critic_rnn_state [N, T / L, A, 128]: the states going into every segment; rnn_seq_len: the storage's
        segment length (must be train_seq_len); last_critic_rnn_state [N, A, 128] and last_is_init [N, 1]: what goes into the step after
        the last one."""
        rk = dict(is_init=is_init, actor_rnn_state=actor_rnn_state, critic_rnn_state=critic_rnn_state, last_critic_rnn_state=last_critic_rnn_state,
                  last_is_init=last_is_init)
        missing = [k for k, v in rk.items() if v is None]
        if missing:
            raise ValueError(f"a recurrent rollout needs {missing} (RolloutStorage.recurrent_kwargs())")
        L = self.train_seq_len
        if rnn_seq_len is not None and int(rnn_seq_len) != L:
            raise ValueError(f"the rollout was stored in segments of {rnn_seq_len} steps, actor.rnn.train_seq_len is {L}")
        N, T = is_init.shape[:2]
        if T % L:
            raise ValueError(f"train_seq_len {L} does not divide the rollout's {T} steps")
        self._check_segments((T // L) * N)
        return self._run(rk, obs_self, obs_others, obs_cylinders, action, log_probs, state_value, next_obs_last, reward, done, agent_done, tp)

    def _check_segments(self, segments):
        if segments < self.num_minibatches:
            raise ValueError(f"the rollout holds {segments} segments, fewer than num_minibatches {self.num_minibatches}")

    def _bootstrap_value(self, next_obs_last, recurrent=None):
        return self.policy.forward(*next_obs_last, critic_state=recurrent["last_critic_rnn_state"], is_init=recurrent["last_is_init"],
                                   value_only=True).value

    # the PPO loop over segments: per epoch one permutation of the N T / L (env, segment) pairs
    def _units(self, N, T):
        return N * (T // self.train_seq_len)

    def _workspaces(self, xs, xc):
        """Every buffer is kept per network; the two gradient buckets are made at the first use on the device."""
        if self.actor_bucket is None:
            self._make_network_buckets()
        return self._rnn_ws

    def _actor_step(self, idx, obs, action, log_probs, adv, rk, **kw):
        return rnn_train.update_actor_rnn(self.actor, *obs, rk["actor_rnn_state"], rk["is_init"], action, log_probs, adv, self.actor_opt, segment=idx,
                                          cfg=self.cfg, seq_len=self.train_seq_len, **kw)

    def _critic_step(self, idx, obs, state_value, ret, rk, **kw):
        return rnn_train.update_critic_rnn(self.critic, *obs, rk["critic_rnn_state"], rk["is_init"], state_value, ret, self.critic_opt, segment=idx,
                                           cfg=self.cfg, seq_len=self.train_seq_len, **kw)


class PerAgentRecurrentDeviceLearner(RecurrentDeviceLearner):
    """MAPPOPolicy's training half with share_actor: False AND actor.rnn / critic.rnn (one actor and one actor GRU per agent, the critic and
    its GRU shared): `RecurrentDeviceLearner`'s blocks in its order, with the actor step through
    rnn_train.update_actor_rnn_per_agent — the encoder op, the GRU op and the head entry on the stacked tensors, ONE gradient bucket, ONE norm
    and ONE ClippedAdam step over the 29 stacked tensors per minibatch.  The critic block, the bootstrap value, the targets, the predictor,
    the info row and state_dict are inherited unchanged.

    actor: the STACKED actor's parameters with their `rnn.*` leaves stacked too (every tensor [A, ...]: the reference's actor_params;
    "actor_params" of state_dict()), live tensors updated in place; device_policy: a PerAgentRecurrentDevicePolicy over the same tensors
    (built when None).  Refused before anything is built: group= (NotImplementedError: DataParallelPerAgentRecurrentLearner's), a
    device_policy that is not both per-agent and recurrent, actor tensors that are not stacked, share_actor: True, and whatever
    PerAgentRecurrentDevicePolicy and the cfg checks of RecurrentDeviceLearner refuse (PolicyConfigError)."""
    stacked_actor = True

    def __init__(self, actor, critic, cfg, tp_net=None, value_normalizer=None, generator=None, device_policy=None, agent_name="drone", group=None):
        if group is not None:
            raise NotImplementedError("PerAgentRecurrentDeviceLearner takes no group=: data-parallel training of recurrent per-agent actors is "
                                      "DataParallelPerAgentRecurrentLearner's")
        if device_policy is not None and not (getattr(device_policy, "per_agent", False) and getattr(device_policy, "recurrent", False)):
            raise P.PolicyConfigError("PerAgentRecurrentDeviceLearner needs a PerAgentRecurrentDevicePolicy (a shared recurrent actor is "
                                      "RecurrentDeviceLearner's, per-agent actors without an rnn PerAgentDeviceLearner's)")
        if not P.is_stacked(actor):
            raise P.PolicyConfigError("PerAgentRecurrentDeviceLearner: the actor's parameters have no leading agent dimension (a shared recurrent "
                                      "actor is RecurrentDeviceLearner's)")
        P.check_config_per_agent(P.cfg_without(cfg, "actor.rnn", "critic.rnn"))
        shared = P.cfg_without(cfg, "share_actor")               # what the shared critic's functions (and policy.check_config behind them) take
        self._build(actor, critic, shared, tp_net, value_normalizer, agent_name, generator, device_policy, P.PerAgentRecurrentDevicePolicy)

    def _actor_step(self, idx, obs, action, log_probs, adv, rk, **kw):
        return rnn_train.update_actor_rnn_per_agent(self.actor, *obs, rk["actor_rnn_state"], rk["is_init"], action, log_probs, adv, self.actor_opt,
                                                    segment=idx, cfg=self.cfg, seq_len=self.train_seq_len, **kw)


class _SegmentCounts:
    """What a data-parallel learner over SEGMENTS replaces in its recurrent parent (DataParallelRecurrentLearner and
    DataParallelPerAgentRecurrentLearner): the rollout's gather counts segments of train_seq_len steps, and the one refusal that depends on
    this rank's count alone moves into that gather's table."""

    def _rollout_counts(self, N, T, A):
        L = self.train_seq_len
        return self._global_counts(N * (T // L), A, unit="segments", rows_per_unit=L, more=(("actor.rnn.train_seq_len", L),))

    def _check_segments(self, segments):
        """Nothing here: a rank with fewer segments than minibatches is refused from the gather's table, on EVERY rank (this rank alone
        raising would leave the others waiting in the gather)."""


class DataParallelRecurrentLearner(_SegmentCounts, RecurrentDeviceLearner):
    """`RecurrentDeviceLearner` over a process group: W ranks, each with the recurrent rollout of its own env slice, perform
    ONE PPO update per minibatch on the union of their minibatches of segments.  group: a torch.distributed process group or "world"
    (required).  What `DeviceLearner(group=)` does for the non-recurrent networks, with the recurrent pieces in place:

        construction, load_state_dict   the group's rank 0 broadcasts both networks (encoder, GRU and head tensors:
                                        rnn_train.flat_parameters), the predictor, ValueNorm1's buffers and the three Adam states
        per train_rollout               one gather of (num_minibatches, ppo_epochs, TP_epochs, predictor on, segments = N T / L, agents,
                                        train_seq_len): all but the segment count must agree and every rank needs one segment per
                                        minibatch, else ValueError on every rank before any further collective;
                                        global_rows = sum_r (segments_r // M) L A
        per minibatch                   each rank permutes its own segments from its own generator; the actor: forward,
                                        hns_rnn_actor_head_grad_global, backward, SUM all-reduce of its bucket, hns_grad_norm, the step; the
                                        critic: forward, hns_rnn_critic_head_sums, SUM all-reduce of five fp64 values,
                                        hns_rnn_critic_head_grad_global, backward, the bucket's all-reduce, the norm, the step — three
                                        collectives per minibatch pair, ONE encoder and GRU pass per network
        predictor, targets, info row    update_tp(group=, bucket=), rollout_targets' gather and _reduce_info, as DeviceLearner(group=):
                                        policy_loss the sum of the shares, ESS the mean of the ranks' own values (a diagnostic),
                                        action_norm the mean over all ranks' rows; every rank returns the same row

    With one rank every parameter and every entry of the info row has RecurrentDeviceLearner's bits."""

    def __init__(self, actor, critic, cfg, tp_net=None, value_normalizer=None, generator=None, device_policy=None, agent_name="drone", group=None):
        if group is None:
            raise ValueError("DataParallelRecurrentLearner needs group=: a torch.distributed process group or \"world\" (one process: "
                             "RecurrentDeviceLearner)")
        super().__init__(actor, critic, cfg, tp_net=tp_net, value_normalizer=value_normalizer, generator=generator, device_policy=device_policy,
                         agent_name=agent_name)
        self._join(group)


class DataParallelPerAgentLearner(PerAgentDeviceLearner):
    """`PerAgentDeviceLearner` over a process group (share_actor: False, data-parallel): what `DeviceLearner(group=)` does for
    the shared actor, with the actor block through actor_train.update_actor_per_agent_global.  group: a torch.distributed process group or
    "world" (required).  Rank 0 broadcasts the 23 STACKED actor tensors, the critic, the predictor, ValueNorm1's buffers and the three Adam
    states; per train_rollout one gather (DeviceLearner(group=)'s table and refusals); per minibatch the actor's
    hns_actor_train_grad_agents_global, the SUM all-reduce of the bucket over the stacked tensors, hns_grad_norm, ONE step; the critic block is
    DeviceLearner(group=)'s, unchanged — three collectives per minibatch pair.  The info row goes through _reduce_info as it is.  With one rank
    every parameter and every entry of the info row is PerAgentDeviceLearner's, as DeviceLearner(group=) is DeviceLearner's."""

    def __init__(self, actor, critic, cfg, tp_net=None, value_normalizer=None, agent_name="drone", generator=None, device_policy=None, group=None):
        if group is None:
            raise ValueError("DataParallelPerAgentLearner needs group=: a torch.distributed process group or \"world\" (one process: "
                             "PerAgentDeviceLearner)")
        super().__init__(actor, critic, cfg, tp_net=tp_net, value_normalizer=value_normalizer, agent_name=agent_name, generator=generator,
                         device_policy=device_policy)
        self._join(group)

    def _actor_step(self, idx, obs, action, log_probs, adv, recurrent, **kw):
        return actor_train.update_actor_per_agent_global(self.actor, *obs, action, log_probs, adv, self.actor_opt, index=idx, cfg=self.cfg, **kw)


class DataParallelPerAgentRecurrentLearner(_SegmentCounts, PerAgentRecurrentDeviceLearner):
    """`PerAgentRecurrentDeviceLearner` over a process group (share_actor: False with actor.rnn / critic.rnn, data-parallel):
    `DataParallelRecurrentLearner`'s construction, gather, collectives and info row, with the actor step through
    rnn_train.update_actor_rnn_per_agent_global — the encoder op, the GRU op and hns_rnn_actor_head_grad_agents_global on the stacked tensors,
    the SUM all-reduce of ONE bucket over the 29 stacked tensors, ONE norm, ONE step.  group: required.  With one rank every parameter and every
    entry of the info row has PerAgentRecurrentDeviceLearner's bits."""

    def __init__(self, actor, critic, cfg, tp_net=None, value_normalizer=None, generator=None, device_policy=None, agent_name="drone", group=None):
        if group is None:
            raise ValueError("DataParallelPerAgentRecurrentLearner needs group=: a torch.distributed process group or \"world\" (one process: "
                             "PerAgentRecurrentDeviceLearner)")
        super().__init__(actor, critic, cfg, tp_net=tp_net, value_normalizer=value_normalizer, generator=generator, device_policy=device_policy,
                         agent_name=agent_name)
        self._join(group)

    def _actor_step(self, idx, obs, action, log_probs, adv, rk, **kw):
        return rnn_train.update_actor_rnn_per_agent_global(self.actor, *obs, rk["actor_rnn_state"], rk["is_init"], action, log_probs, adv, self.actor_opt,
                                                           segment=idx, cfg=self.cfg, seq_len=self.train_seq_len, **kw)
