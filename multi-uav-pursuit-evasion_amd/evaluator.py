"""Evaluation on the device: the `evaluate()` of scripts/train.py:207-264 — a seeded, deterministic rollout of max_episode_length steps, each
env's statistics at its first `done`, `nanmean`ed into `eval/stats.*` — without the reference's per-step stacking.

`DeviceEvaluator(env, policy).evaluate(seed)` clears what a reset would carry over from earlier episodes (`env.clear_carried_state()`: the
reference's `_reset_idx` leaves the rate controller's integrator, part of `prev_action` and the predictor's window alone, so its evaluate()
depends on what the env ran before; here a run is a function of the seed and the networks), resets every env, then runs L = env.max_episode_length times `policy.act` (hns_policy_act: the
actor alone, the mode of the distribution, into ONE persistent action tensor) and `env.step` on ONE persistent tensordict, through the public
calls only, so an env subclass keeps its hooks.  Nothing is stored per step: `done` is pure truncation (the rule hns_amd.collector rests on),
so after a full reset every env is done exactly at step L, and each env's statistics at its first done are simply the statistics after the
last step.  One launch of hns_eval_means then turns them into the NaN-skipping means over the done envs; means and counts come to the host
in ONE copy, the run's only host synchronisation.  An env that is not done after L steps breaks the rule and raises (the reference would
quietly take its statistics of step 0, `argmax` over an all-false row).

Training is left as it was: the env's `training` flag, seed and reset epoch, torch's CPU generator and the env device's generator are put
back (`env.set_seed` calls `torch.manual_seed`), and a collector on the same env is told to `restart()`.  With `tp_net` the predictor's
current parameters are copied into the evaluated env's own first — evaluate on a separate env of any size and training never notices.

On a HideAndSeek_envgen the run's last step triggers the generator's episode-end hook, as it does in the reference, and the generator's
own state is not restored: evaluate on a separate env if that matters.

CPU tensors and stub envs take `stat_means`, the kernel's definition restated on the host (tests; not the hot path).  DESIGN.md §7.8."""
import ctypes as C

import numpy as np
import torch

from . import abi
from .env import HnsError
from .tensordict_shim import TensorDict

KEY = "eval/stats."
_THREADS = 256


def stat_means(values, mask=None):
    """hns_eval_means on the host: values [S, N] (or a list of S rows of N), mask [N] or None -> (mean [S] float32, used [S] int64, masked).
    Row i's mean is taken over the envs e with mask[e] != 0 of the values that are not NaN, used[i] counts them, `masked` counts the envs;
    no value entering gives NaN.  The sum runs in the kernel's order — 256 fp64 partials over e = t, t + 256, ..., a fixed-order tree, one
    division, one rounding to fp32 — so the device gives the same bits."""
    m = None if mask is None else np.asarray(torch.as_tensor(mask).detach().cpu().reshape(-1).numpy()) != 0
    if len(values) == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.int64), int(m.sum()) if m is not None else 0
    v = np.stack([np.asarray(torch.as_tensor(r).detach().cpu().reshape(-1).numpy(), dtype=np.float32) for r in values])
    S, N = v.shape
    m = np.ones(N, bool) if m is None else m
    if m.shape != (N,):
        raise ValueError(f"mask must have {N} entries, not {m.shape[0]}")
    enter = m[None, :] & ~np.isnan(v)
    x = np.where(enter, v, np.float32(0.0)).astype(np.float64)                 # (adding 0.0 to a partial leaves it as it is)
    pad = (-N) % _THREADS
    part = np.pad(x, ((0, 0), (0, pad))).reshape(S, -1, _THREADS)
    s = np.zeros((S, _THREADS), np.float64)
    with np.errstate(invalid="ignore"):                                        # inf + -inf = NaN is the definition, not a mistake
        for chunk in range(part.shape[1]):                                     # partial t: its elements in index order
            s = s + part[:, chunk]
        half = _THREADS // 2
        while half:                                                            # partial t takes partial t + half
            s = s[:, :half] + s[:, half:2 * half]
            half //= 2
    used = enter.sum(1).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(used > 0, s[:, 0] / np.maximum(used, 1), np.nan).astype(np.float32)
    return mean, used, int(m.sum())


class DeviceEvaluator:
    """env: a HideAndSeek (or a subclass, or anything with its set_seed / reset / step / stats / max_episode_length surface); policy: a
    DevicePolicy (anything with `act(state_self, state_others, cylinders, out=None)`), or a recurrent policy: one whose `recurrent` attribute
    is true (RecurrentDevicePolicy) must offer `act_step(state_self, state_others, cylinders, state=None, is_init=None, out=None,
    out_state=None) -> (action, state)` with state=None meaning zeros and `out_state` allowed to be `state`; the run then owns ONE persistent
    [N, A, 128] actor state beside its one action tensor — zeros going into step 0 (the full reset), carried in place from then on, nothing
    stored per step, the policy's call counter and a collector's own rnn states untouched.  tp_net: the predictor whose parameters the env's own
    `TP` takes before a run (the training env's, when `env` is a separate evaluation env).  collector: a DeviceCollector ON THIS env, told to
    `restart()` after every run.

    After a run `stats` is {name: [N] tensor}, each env's statistics at its first done (a clone); `steps` and `done_reads` count the env
    steps and the host read-backs made so far."""

    def __init__(self, env, policy, tp_net=None, collector=None):
        if collector is not None and collector.env is not env:
            raise ValueError("the collector runs on another env: pass the collector of the env that is evaluated, or none")
        self.env, self.policy, self.tp_net, self.collector = env, policy, tp_net, collector
        self.stats = None
        self.steps = self.done_reads = 0
        self.launches = 0                                        # hns_eval_means calls made (tools/eval_cost.py)

    # ---- what a run must not leave behind
    def _save(self):
        env = self.env
        dev = getattr(env, "device", None)
        cuda = isinstance(dev, torch.device) and dev.type == "cuda"
        return {"training": getattr(env, "training", None), "seed": getattr(env, "seed", None), "epoch": getattr(env, "reset_epoch", None),
                "cpu_rng": torch.get_rng_state(), "dev_rng": torch.cuda.get_rng_state(dev) if cuda else None,
                "render": getattr(env, "_render", None)}

    def _restore(self, saved):
        env = self.env
        if saved["training"] is not None:
            if hasattr(env, "train"):
                env.train(saved["training"])
            else:
                env.training = saved["training"]
        if saved["seed"] is not None:
            env.seed = saved["seed"]                             # (not set_seed: that would seed torch and clear the reset epoch again)
        if saved["epoch"] is not None:
            if hasattr(env, "set_reset_epoch"):
                env.set_reset_epoch(saved["epoch"])
            else:
                env.reset_epoch = saved["epoch"]
        if saved["render"] is not None and hasattr(env, "enable_render") and getattr(env, "_render", None) is not saved["render"]:
            env.enable_render(saved["render"])
        torch.set_rng_state(saved["cpu_rng"])
        if saved["dev_rng"] is not None:
            torch.cuda.set_rng_state(saved["dev_rng"], env.device)

    def _take_predictor(self):
        own = getattr(self.env, "TP", None)
        if self.tp_net is None or self.tp_net is own:
            return
        if own is None:
            raise ValueError("tp_net was given, but the env has no predictor (algo.use_TP_net: 0)")
        src = self.tp_net.state_dict()
        with torch.no_grad():
            for k, v in own.state_dict().items():                # in place: the version counters move and the env re-packs
                v.copy_(src[k])

    @staticmethod
    def _obs(td):
        obs = td[("agents", "observation")]
        return obs["state_self"], (obs.get("state_others", None) if hasattr(obs, "get") else None), obs["cylinders"]

    # ---- the run
    def evaluate(self, seed=0, frame_every=0):
        """{"eval/stats.<name>": float} (the reference's keys, train.py:251-254); frame_every > 0 also returns "frames", a uint8 array
        [F, 3, H, W] of env.render(mode="rgb_array") after every frame_every-th step (each frame is a host read: off by default)."""
        env = self.env
        saved = self._save()
        frames = []
        try:
            if hasattr(env, "train"):
                env.train(True)                                  # the outputs are views of the env's buffers: no per-step clones
            else:
                env.training = True
            if frame_every > 0 and hasattr(env, "enable_render"):
                env.enable_render(True)
            self._take_predictor()
            env.set_seed(seed)
            if hasattr(env, "clear_carried_state"):
                env.clear_carried_state()                        # what a reset leaves alone (controller state, the predictor's window) must
            cur = env.reset()                                    # not make the run depend on what the env did before it
            action = step_td = state = None
            recurrent = getattr(self.policy, "recurrent", False)
            for t in range(int(env.max_episode_length)):
                if recurrent:                                    # state None at step 0: zeros, the full reset; then in place
                    action, state = self.policy.act_step(*self._obs(cur), state=state, out=action, out_state=state)
                else:
                    action = self.policy.act(*self._obs(cur), out=action)
                if step_td is None:
                    step_td = TensorDict({"agents": {"action": action}}, env.batch_size)
                cur = env.step(step_td)["next"]
                self.steps += 1
                if frame_every > 0 and t % frame_every == 0:
                    frames.append(env.render(mode="rgb_array"))
            out = self._means(cur["done"], env.stats)
        finally:
            self._restore(saved)
            if self.collector is not None:
                self.collector.restart()
        if frames:
            out["frames"] = np.stack(frames).transpose(0, 3, 1, 2)
        return out

    def _means(self, done, stats):
        n = done.numel()
        names = [k for k in stats.keys() if torch.is_tensor(stats[k]) and stats[k].numel() == n]
        mask = done.reshape(-1).clone()
        if not names:
            rows = torch.zeros(0, n)
        else:
            rows = torch.stack([stats[k].reshape(-1).float() for k in names])            # the clone: one copy of every statistic, [S, N]
        self.stats = {k: rows[i] for i, k in enumerate(names)}
        if rows.device.type == "cuda" and names:
            mean, masked = self._device_means(rows, mask)
        else:
            mean, _, masked = stat_means(rows, mask)
            self.done_reads += 1
        if masked != n:
            raise HnsError(f"{n - masked} of {n} envs were not done after max_episode_length = {int(self.env.max_episode_length)} steps from a "
                           "full reset: `done` must be pure truncation (every env done exactly then); their first-episode statistics do not "
                           "exist")
        return {KEY + k: float(m) for k, m in zip(names, mean)}

    def _device_means(self, rows, mask):
        """hns_eval_means over the rows of `rows` [S, N] (64 per launch), mask uint8 [N]; every launch's means and counts in ONE int64 buffer
        — per launch of c rows: used [c + 1], then the c fp32 means in (c + 1) // 2 words — that crosses to the host in one copy."""
        S, N = rows.shape
        M = abi.HNS_EVAL_MAX_ROWS
        chunks = [(s, min(M, S - s)) for s in range(0, S, M)]
        words = sum(c + 1 + (c + 1) // 2 for _, c in chunks)
        buf = torch.empty(words, dtype=torch.int64, device=rows.device)
        mask8 = mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8)
        lib, at, where = abi.load_library(), 0, []
        with torch.cuda.device(rows.device):
            st = C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)
            for s, c in chunks:
                table = (abi.HnsEvalRow * M)()
                for i in range(c):
                    table[i].src, table[i].stride = rows[s + i].data_ptr(), rows.stride(1)
                used, mean = buf[at:at + c + 1], buf[at + c + 1:at + c + 1 + (c + 1) // 2]
                abi.check(lib.hns_eval_means(table, c, N, mask8.data_ptr(), mean.data_ptr(), used.data_ptr(), st), "hns_eval_means")
                self.launches += 1
                where.append((at, c))
                at += c + 1 + (c + 1) // 2
        host = buf.cpu().numpy()                                 # the run's one host synchronisation
        self.done_reads += 1
        means = np.concatenate([host[a + c + 1:a + c + 1 + (c + 1) // 2].view(np.float32)[:c] for a, c in where])
        return means, int(host[where[0][0] + where[0][1]])
