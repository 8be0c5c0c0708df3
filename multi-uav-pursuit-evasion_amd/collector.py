"""The rollout collector: env -> policy -> learner-ready storage, the loop the reference gets from SyncDataCollector(..., return_same_td=True)
(scripts/train.py:196-205) feeding MAPPOPolicy.train_op.

`RolloutStorage(num_envs, num_steps, example)` preallocates batch-major [N, T, ...] tensors (and [N, ...] ones for the last step's next
observation) and `store(slot, {name: tensor})` writes one time slot of several of them in ONE launch of hns_rollout_store — as torch `copy_`
calls that is a launch per tensor.  The destination half of the segment list is built once per set of names; the source pointers are
filled in per call.  `learner_kwargs()` hands the storage to `DeviceLearner.train_rollout` as views, no copy.

`DeviceCollector(env, policy, num_steps).collect()` runs num_steps steps through the public calls only (`env.reset(td)`, `env.step(td)`,
`policy.forward`), so an env subclass keeps its host hooks.  Per step t:

    policy      on the current observation
    store       observation keys, action, log-prob, value -> slot t   BEFORE the step: the step rewrites the observation buffers in place
    env.step
    store       reward, done, the predictor's entries -> slot t       BEFORE any reset: the reset clears `done` and rewrites the buffers
                (at t = T - 1 also the next observation -> next_obs_last)
    env.reset   of exactly the done envs, if any

No env can be done before max_episode_length steps have passed since the last reset that covered every env, so `done` is read back to the
host only from then on: with lock-step episodes one read per episode, not one per step.  The statistics `reset` returns (the values from
before the reset) are summed over the done envs on the device; `episode_stats()` brings the means across in one copy.

With a recurrent policy (`policy.recurrent`: RecurrentDevicePolicy) the collector also owns the two rnn states, which the
policy updates in place, and an env-level `is_init` buffer: all ones after a full reset, the reset mask on the step after a partial reset,
and otherwise not handed to the kernel at all.  The storage gains `is_init` [N, T, 1] (in the pre-step store) and, per segment of
`rnn_seq_len` steps, the two states going INTO the segment's first step ([N, T / rnn_seq_len, A, 128], stored before the policy call); the
last step's next `is_init` (its `done`) and critic state join `next_obs_last`.  `recurrent_kwargs()` hands them out.  A non-recurrent policy
takes none of this: the same calls, launches and bits as before.

With a policy that reads the state (`policy.needs_state`: CentralCriticDevicePolicy, critic_input: state) the collector reads
("agents", "state", "state_drones") each step, hands it to `forward` and stores it as `state_drones` [N, T, A, D] — one more segment of the
pre-step store, not one more launch — and the last step's next one beside `next_obs_last`; `learner_kwargs()` gains `state_drones` and
`next_state_last`.  The state's cylinders are agent 0's rows of the stored obs_cylinders: no second copy is stored.  Every other policy takes
none of this.

CPU tensors take plain indexing assignment (tests; not the hot path).  DESIGN.md §7.7."""
import ctypes as C

import numpy as np
import torch

from . import abi
from .tensordict_shim import TensorDict

OBS_KEYS = (("obs_self", "state_self"), ("obs_others", "state_others"), ("obs_cylinders", "cylinders"))      # storage name, observation key
TP_KEYS = ("TP_input", "TP_groundtruth", "TP_done")
LAST_NAMES = tuple(n for n, _ in OBS_KEYS)
RNN_STATES = ("actor_rnn_state", "critic_rnn_state")
STATE_NAME = "state_drones"                                     # storage name and key under ("agents", "state") of what a centralised critic reads
RNN_LAST_NAMES = LAST_NAMES + ("critic_rnn_state", "is_init")   # what the bootstrap value of a recurrent critic needs beside the observation


class RolloutStorage:
    """example: {name: tensor [N, ...]} — every name gets an [N, T, ...] tensor of that dtype and trailing shape on that device (bool stays
    bool); the names in `last` also get an [N, ...] tensor, written by `store_last` (the last step's next observation)."""

    def __init__(self, num_envs, num_steps, example, last=LAST_NAMES):
        if num_envs < 1 or num_steps < 1:
            raise ValueError("num_envs and num_steps must be >= 1")
        self.num_envs, self.num_steps = int(num_envs), int(num_steps)
        self.data, self.last, self.segments = {}, {}, {}
        self.rnn_seq_len = None
        self._last_names = tuple(last)
        self._plans = {}
        self.launches = 0                                        # hns_rollout_store calls made (tools/collector_cost.py)
        self.allocate(example)

    def allocate(self, example):
        """Add storage for more names (the collector learns the post-step entries' shapes from its first step)."""
        N, T = self.num_envs, self.num_steps
        for name, t in example.items():
            if name in self.data:
                raise KeyError(f"{name} is already allocated")
            if t.dim() < 1 or t.shape[0] != N:
                raise ValueError(f"{name}: the example must be [{N}, ...], not {tuple(t.shape)}")
            self.data[name] = torch.zeros(N, T, *t.shape[1:], dtype=t.dtype, device=t.device)
            if name in self._last_names:
                self.last[name] = torch.zeros(N, *t.shape[1:], dtype=t.dtype, device=t.device)

    def allocate_segments(self, example, seq_len):
        """Per-segment storage [N, T / seq_len, ...] for `example`'s names (the rnn states going into every segment's first step); the
        names in `last` also get their [N, ...] tensor."""
        N, T = self.num_envs, self.num_steps
        if seq_len < 1 or T % seq_len:
            raise ValueError(f"the segment length {seq_len} must divide num_steps {T}")
        self.rnn_seq_len = int(seq_len)
        for name, t in example.items():
            if name in self.segments or name in self.data:
                raise KeyError(f"{name} is already allocated")
            if t.dim() < 1 or t.shape[0] != N:
                raise ValueError(f"{name}: the example must be [{N}, ...], not {tuple(t.shape)}")
            self.segments[name] = torch.zeros(N, T // seq_len, *t.shape[1:], dtype=t.dtype, device=t.device)
            if name in self._last_names:
                self.last[name] = torch.zeros(N, *t.shape[1:], dtype=t.dtype, device=t.device)

    # ---- writes
    def store(self, slot, tensors):
        """tensors[name] [N, ...] -> data[name][:, slot], every other slot untouched."""
        if not 0 <= slot < self.num_steps:
            raise IndexError(f"slot {slot} outside [0, {self.num_steps})")
        self._store(self.data, int(slot), self.num_steps, tensors)

    def store_last(self, tensors):
        """tensors[name] [N, ...] -> last[name]."""
        self._store(self.last, 0, 1, tensors)

    def store_segment(self, segment, tensors):
        """tensors[name] [N, ...] -> segments[name][:, segment]."""
        num = self.num_steps // self.rnn_seq_len if self.rnn_seq_len else 0
        if not 0 <= segment < num:
            raise IndexError(f"segment {segment} outside [0, {num})")
        self._store(self.segments, int(segment), num, tensors)

    def _store(self, where, slot, num_slots, tensors):
        items = [(k, v) for k, v in tensors.items() if v is not None]
        slotted = where is not self.last
        for name, t in items:
            dst = where[name]
            want = dst.shape[:1] + dst.shape[(2 if slotted else 1):]
            if t.shape != want or t.dtype != dst.dtype or t.device != dst.device:
                raise ValueError(f"{name}: expected {dst.dtype} {tuple(want)} on {dst.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        if not items:
            return
        if items[0][1].device.type != "cuda":
            for name, t in items:
                if slotted:
                    where[name][:, slot] = t
                else:
                    where[name].copy_(t)
            return
        # the destination half of the segment list is fixed per set of names and built once; the sources may move between calls (a policy's
        # outputs are fresh tensors every step), so their pointers are filled in per call and a changed stride rebuilds the plan
        key = (0 if where is self.data else 1 if where is self.last else 2, tuple(name for name, _ in items))
        plan = self._plans.get(key)
        if plan is None or any(t.stride() != s for (_, t), s in zip(items, plan[3])):
            plan = self._plans[key] = self._plan(where, num_slots, items)
        segments, fused, loose, _ = plan
        for n, i in enumerate(fused):
            segments[n].src = items[i][1].data_ptr()
        dev = items[0][1].device
        for i in loose:                                          # a per-env block that is not contiguous: this tensor alone goes through copy_
            name, t = items[i]
            (where[name][:, slot] if slotted else where[name]).copy_(t)
        if fused:
            with torch.cuda.device(dev):
                rc = abi.load_library().hns_rollout_store(segments, len(fused), self.num_envs, slot, num_slots,
                                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            abi.check(rc, "hns_rollout_store")
            self.launches += 1

    def _plan(self, where, num_slots, items):
        """(segment array, indices of the tensors in it, indices of those left to copy_, the sources' strides) for this set of names."""
        if len(items) > abi.HNS_ROLLOUT_MAX_SEGMENTS:
            raise ValueError(f"{len(items)} tensors in one store, at most {abi.HNS_ROLLOUT_MAX_SEGMENTS}")
        segments, fused, loose = (abi.HnsRolloutSegment * abi.HNS_ROLLOUT_MAX_SEGMENTS)(), [], []
        for i, (name, t) in enumerate(items):
            dst = where[name]
            row = t[0].numel() * t.element_size()
            if row == 0:
                continue
            if not t[0].is_contiguous() or (self.num_envs > 1 and t.stride(0) * t.element_size() < row):
                loose.append(i)
                continue
            s = segments[len(fused)]
            s.dst = dst.data_ptr()
            s.src_stride = max(t.stride(0) * t.element_size(), row)           # (one env: any stride a view may carry)
            s.dst_stride, s.row_bytes = num_slots * row, row
            fused.append(i)
        return segments, fused, loose, [t.stride() for _, t in items]

    # ---- the learner's view
    def learner_kwargs(self):
        """The keyword arguments of DeviceLearner.train_rollout, as views of the storage."""
        d, l = self.data, self.last
        kw = {"obs_self": d["obs_self"], "obs_others": d.get("obs_others"), "obs_cylinders": d["obs_cylinders"], "action": d["action"],
              "log_probs": d["log_probs"], "state_value": d["state_value"],
              "next_obs_last": (l["obs_self"], l.get("obs_others"), l["obs_cylinders"]), "reward": d["reward"], "done": d["done"]}
        if "TP_input" in d:
            kw["tp"] = tuple(d[k] for k in TP_KEYS)
        if STATE_NAME in d:                                      # a centralised critic's (CentralCriticDeviceLearner.train_rollout)
            kw["state_drones"], kw["next_state_last"] = d[STATE_NAME], l[STATE_NAME]
        return kw

    def recurrent_kwargs(self):
        """What training a recurrent policy needs beside learner_kwargs(), as views of the storage: `is_init` [N, T, 1]; the two states going
        into the first step of every `rnn_seq_len`-step segment [N, T / rnn_seq_len, A, 128]; the critic state and `is_init` going into the
        step after the last one (the bootstrap value: one value_only call on next_obs_last)."""
        if not self.segments:
            raise KeyError("this storage holds no rnn state (the collector's policy is not recurrent)")
        return {"is_init": self.data["is_init"], "actor_rnn_state": self.segments["actor_rnn_state"],
                "critic_rnn_state": self.segments["critic_rnn_state"], "rnn_seq_len": self.rnn_seq_len,
                "last_critic_rnn_state": self.last["critic_rnn_state"], "last_is_init": self.last["is_init"]}


def _get(td, key):
    return td.get(key, None) if hasattr(td, "get") else td[key]


class DeviceCollector:
    """env: a HideAndSeek (or a subclass, or anything with its reset / step / max_episode_length surface); policy: a DevicePolicy (anything
    whose forward(state_self, state_others, cylinders) returns .action, .log_prob, .value).  The current observation is carried from one
    collect() to the next; the first call does the full reset.

    The read-back rule rests on the collector's own step count, so two things must hold of the env: (1) an env is done only by reaching
    max_episode_length steps since its reset (pure truncation, as HideAndSeek's step decides it: no early termination), and (2) between
    collect() calls nobody else steps, resets or loads a state into the env — or, where somebody did (an evaluation on the same env:
    hns_amd.evaluator), `restart()` is called before the next collect().  An env that can end an episode early, or that is driven from
    outside as well, needs a loop that reads `done` on every step."""

    def __init__(self, env, policy, num_steps, rnn_seq_len=None):
        if num_steps < 1:
            raise ValueError("num_steps must be >= 1")
        self.env, self.policy, self.num_steps = env, policy, int(num_steps)
        self.recurrent = bool(getattr(policy, "recurrent", False))
        self.needs_state = bool(getattr(policy, "needs_state", False))
        if self.recurrent and self.needs_state:
            raise ValueError("a recurrent policy that reads the state is not supported")
        if self.recurrent:
            self.rnn_seq_len = 16 if rnn_seq_len is None else int(rnn_seq_len)          # the reference's train_seq_len
            if self.rnn_seq_len < 1 or self.num_steps % self.rnn_seq_len:
                raise ValueError(f"rnn_seq_len {self.rnn_seq_len} must divide num_steps {self.num_steps}")
        elif rnn_seq_len is not None:
            raise ValueError("rnn_seq_len is for a recurrent policy (policy.recurrent)")
        self._states = self._is_init = None                     # recurrent: (actor, critic) [N, A, 128], updated in place; [N, 1] bool
        self._init_pending = False                               # the buffer holds a flag: the next policy call reads it
        self.max_episode_length = int(env.max_episode_length)
        self.storage = None
        self._cur = None
        self._step_td = None
        self._since_full_reset = 0
        self.done_reads = 0                                      # host read-backs of `done` so far
        self._stat_keys = self._stat_sum = None
        self._episodes = 0

    def restart(self):
        """Drop the carried observation: the next collect() begins with a full reset, as the first one did (after somebody else drove the env)."""
        self._cur = None

    @staticmethod
    def _obs(td):
        obs = td[("agents", "observation")]
        return {name: _get(obs, key) for name, key in OBS_KEYS}

    @staticmethod
    def _state(td):
        return td[("agents", "state")][STATE_NAME]

    def _done_count(self, done):
        """The loop's one host read-back: how many envs are done."""
        self.done_reads += 1
        return int(done.sum())

    def collect(self):
        """num_steps steps into the storage; returns it (the same object every call)."""
        env, T = self.env, self.num_steps
        full_reset = self._cur is None
        if full_reset:
            self._cur = env.reset()
            self._since_full_reset = 0
        cur = self._cur
        if self.recurrent and full_reset:
            self._rnn_begin(self._obs(cur)["obs_self"])
        for t in range(T):
            obs = self._obs(cur)
            if self.recurrent:
                out, rnn_pre = self._rnn_forward(t, obs)
            elif self.needs_state:                               # (rnn_pre: what joins the pre-step store beside the observation)
                rnn_pre = {STATE_NAME: self._state(cur)}
                out = self.policy.forward(obs["obs_self"], obs["obs_others"], obs["obs_cylinders"], rnn_pre[STATE_NAME])
            else:
                out, rnn_pre = self.policy.forward(obs["obs_self"], obs["obs_others"], obs["obs_cylinders"]), {}
            pre = {**obs, "action": out.action, "log_probs": out.log_prob, "state_value": out.value, **rnn_pre}
            if self.storage is None:
                n = obs["obs_self"].shape[0]
                self.storage = RolloutStorage(n, T, {k: v for k, v in pre.items() if v is not None},
                                              last=RNN_LAST_NAMES if self.recurrent else LAST_NAMES + (STATE_NAME,) if self.needs_state else LAST_NAMES)
                if self.recurrent:
                    self.storage.allocate_segments(dict(zip(RNN_STATES, self._states)), self.rnn_seq_len)
            self.storage.store(t, pre)
            if self._init_pending:                               # the flags were for this step alone
                self._is_init.zero_()
                self._init_pending = False
            if self._step_td is None:
                self._step_td = TensorDict({"agents": {"action": out.action}}, env.batch_size)
            else:
                self._step_td.set(("agents", "action"), out.action)
            nxt = env.step(self._step_td)["next"]
            done = nxt["done"]
            post = {"reward": nxt[("agents", "reward")], "done": done}
            tp = _get(nxt["agents"], "TP")
            if tp is not None:
                post.update({k: tp[k] for k in TP_KEYS})
            if "reward" not in self.storage.data:
                self.storage.allocate(post)
            self.storage.store(t, post)
            if t == T - 1:
                # (recurrent: the next step's is_init is this step's done, and the reset below leaves the states alone)
                self.storage.store_last({**self._obs(nxt), "critic_rnn_state": self._states[1], "is_init": done} if self.recurrent
                                        else {**self._obs(nxt), STATE_NAME: self._state(nxt)} if self.needs_state else self._obs(nxt))
            cur = nxt
            self._since_full_reset += 1
            if self._since_full_reset >= self.max_episode_length:
                n_done = self._done_count(done)
                if n_done:
                    mask = done.clone()                          # (`done` is the env's buffer: the reset clears it)
                    cur = env.reset(TensorDict({"_reset": mask}, env.batch_size))
                    if self.recurrent:
                        self._is_init.copy_(mask.reshape(self._is_init.shape))
                        self._init_pending = True
                    self._add_stats(_get(cur, "stats"), mask, n_done)
                    if n_done == done.numel():
                        self._since_full_reset = 0
        self._cur = cur
        return self.storage

    # ---- the recurrent policy's state
    def _rnn_begin(self, obs_self):
        """After a full reset: every env starts an episode (the states are masked by the flag, whatever they hold)."""
        if self._states is None:
            n, a = obs_self.shape[:2]
            self._states = tuple(torch.zeros(n, a, abi.HNS_GRU_HIDDEN, dtype=torch.float32, device=obs_self.device) for _ in range(2))
            self._is_init = torch.zeros(n, 1, dtype=torch.bool, device=obs_self.device)
        self._is_init.fill_(True)
        self._init_pending = True

    def _rnn_forward(self, t, obs):
        """The policy call of step t: the states going into a segment's first step are stored first (the call updates them in place)."""
        # (the storage is made after the first step ever; the states are zeros then, which is what the fresh storage holds)
        if t % self.rnn_seq_len == 0 and self.storage is not None:
            self.storage.store_segment(t // self.rnn_seq_len, dict(zip(RNN_STATES, self._states)))
        out = self.policy.forward(obs["obs_self"], obs["obs_others"], obs["obs_cylinders"], actor_state=self._states[0],
                                  critic_state=self._states[1], is_init=self._is_init if self._init_pending else None, out_states=self._states)
        return out, {"is_init": self._is_init}

    # ---- episode statistics
    def _add_stats(self, stats, done, n_done):
        self._episodes += n_done
        if stats is None:
            return
        if self._stat_keys is None:
            self._stat_keys = [k for k in stats.keys() if torch.is_tensor(stats[k]) and stats[k].numel() == done.numel()]
            self._stat_sum = torch.zeros(len(self._stat_keys), dtype=torch.float64, device=done.device)
        if not self._stat_keys:
            return
        vals = torch.stack([stats[k].reshape(-1) for k in self._stat_keys]).double()
        self._stat_sum += torch.where(done.reshape(1, -1), vals, torch.zeros((), dtype=torch.float64, device=vals.device)).sum(1)

    def episode_stats(self):
        """({statistic: its mean over the episodes that ended since the last call}, their number) — the fp64 sums divided once and rounded
        once to fp32, one copy to the host; then cleared."""
        n, keys = self._episodes, self._stat_keys or []
        means = {}
        if n and keys:
            means = {k: float(np.float32(v)) for k, v in zip(keys, (self._stat_sum / n).tolist())}
            self._stat_sum.zero_()
        self._episodes = 0
        return means, n
