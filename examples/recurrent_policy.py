#!/usr/bin/env python3
"""A recurrent actor and critic — the reference's `actor.rnn` / `critic.rnn` configuration — collected on the device and trained in torch:

    python examples/recurrent_policy.py --envs 256 --steps 32 --updates 4          # on the device: HideAndSeek, RecurrentDevicePolicy in one launch per step
    python examples/recurrent_policy.py --envs 4 --steps 32 --updates 2            # without a GPU: a seeded stand-in env, the torch restatements

Collection: `DeviceCollector(env, RecurrentDevicePolicy, steps, rnn_seq_len=16)`.  The policy reads the training modules' parameters in place
(their tensors under the reference's names), so the next collect() follows the optimiser's steps.  The storage holds, beside the rollout,
`is_init` per step and the two rnn states going INTO every 16-step segment (`recurrent_kwargs()`).

Training: each network is AttentionEncoder -> GRU -> a torch head (hns_amd.encoder, hns_amd.rnn: HIP forward and backward under autograd).
A minibatch is a set of (env, segment) pairs; a segment starts from its STORED state, the stored flags mask the state inside it, so the
recomputed log-probabilities are the collected ones up to rounding: the script prints max |ratio - 1| of the first minibatch before any step.
The losses are the reference's clipped PPO surrogate with an entropy bonus and the clipped Huber value loss; the targets come from
gae.rollout_targets with the bootstrap value of ONE value_only call on the last next observation, the stored last critic state and flags.

--learner: train through `learner.RecurrentDeviceLearner` instead of the torch loop below — one `train_rollout` per rollout (the bootstrap
value, the targets, the env's trajectory predictor (on the device), `--updates` PPO epochs of 4 minibatches of segments through rnn_train.update_actor_rnn / update_critic_rnn: the head and
the loss in HIP too, two optimisers, no host synchronisation in the loop) — and print the reference's info row.  Under a launcher
(WORLD_SIZE set) the script is then one rank of a data-parallel run: --envs is the WHOLE job's env count, each rank steps its
`sharding.env_shard` slice, `learner.DataParallelRecurrentLearner(group="world")` performs one update on the union of the ranks' minibatches,
and rank 0 alone prints.  The backend is HNS_DIST_BACKEND (default nccl, RCCL on ROCm; gloo runs several ranks on one card as a correctness run).

--eval: after training, one seeded deterministic episode through `DeviceEvaluator(env, pol, collector=col)` — the actor alone with its state
carried on the device (`RecurrentDevicePolicy.act_step`), the `eval/stats.*` means printed."""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hns_amd  # noqa: E402,F401
from hns_amd import collector, evaluator, gae, policy, sharding  # noqa: E402
from hns_amd.encoder import AttentionEncoder  # noqa: E402
from hns_amd.learner import DataParallelRecurrentLearner, RecurrentDeviceLearner, ValueNorm1  # noqa: E402
from hns_amd.rnn import GRU  # noqa: E402
from hns_amd.tensordict_shim import TensorDict  # noqa: E402

SEQ = 16                                                        # cfg/algo/mappo.yaml: train_seq_len


class Network(nn.Module):
    """encoder -> GRU -> head; `names` maps the reference's parameter names to this module's tensors (what RecurrentDevicePolicy parses)."""

    def __init__(self, D, A, actor, seed):
        super().__init__()
        self.encoder, self.rnn = AttentionEncoder(D, A, seed=seed), GRU()
        self.head = nn.Linear(128, 4 if actor else 1)
        nn.init.orthogonal_(self.head.weight, 0.01)
        nn.init.zeros_(self.head.bias)
        self.log_std = nn.Parameter(torch.zeros(4)) if actor else None

    def names(self):
        enc, head = ("encoder.", "act_dist.fc_mean.") if self.log_std is not None else ("base.", "v_out.")
        out = {enc + k: v for k, v in self.encoder.named_parameters()}
        out.update({"rnn." + k: v for k, v in self.rnn.named_parameters()})
        out.update({head + "weight": self.head.weight, head + "bias": self.head.bias})
        if self.log_std is not None:
            out["act_dist.log_std"] = self.log_std
        return out

    def forward(self, obs, index, h0, flags, B, A):
        x = self.encoder(*obs, index, check_index=False).view(B, SEQ, A, 128).transpose(1, 2)      # [B, A, SEQ, 128]: a view, read in place
        out, _ = self.rnn(x, h0, flags)
        return self.head(out).transpose(1, 2).reshape(B * SEQ, A, -1)


class StandInEnv:
    """Without a GPU: seeded random observations behind HideAndSeek's reset / step surface, lock-step episodes of `max_episode_length`.
    For --eval: `set_seed` and one per-env statistic, the episode's sum of |action|."""

    def __init__(self, envs, A=3, K=5, D=35, max_episode_length=24):
        self.n, self.A, self.K, self.D = envs, A, K, D
        self.batch_size, self.max_episode_length = torch.Size([envs]), max_episode_length
        self.g = torch.Generator().manual_seed(0)
        self.progress = torch.zeros(envs, dtype=torch.long)
        self.stats = {"action_sum": torch.zeros(envs, 1)}

    def set_seed(self, seed=-1):
        self.g.manual_seed(seed)

    def _td(self):
        rn = lambda *s: torch.randn(*s, generator=self.g)
        obs = {"state_self": 0.7 * rn(self.n, self.A, 1, self.D), "state_others": 0.5 * rn(self.n, self.A, self.A - 1, 3),
               "cylinders": 0.5 * rn(self.n, self.A, self.K, 5)}
        return TensorDict({"agents": {"observation": obs}}, self.batch_size)

    def reset(self, td=None):
        mask = torch.ones(self.n, dtype=torch.bool) if td is None else td["_reset"].reshape(-1)
        self.progress[mask] = 0
        self.stats["action_sum"][mask] = 0
        return self._td()

    def step(self, td):
        self.progress += 1
        self.stats["action_sum"] += td[("agents", "action")].abs().sum((1, 2)).reshape(self.n, 1)
        nxt = self._td()
        nxt.set(("agents", "reward"), 0.1 * torch.randn(self.n, self.A, 1, generator=self.g))
        nxt.set("done", (self.progress >= self.max_episode_length).reshape(self.n, 1))
        td.set("next", nxt)
        return td

    def close(self):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--updates", type=int, default=4)
    ap.add_argument("--learner", action="store_true", help="train through RecurrentDeviceLearner (one train_rollout per rollout) instead of the torch loop")
    ap.add_argument("--eval", action="store_true", help="after training: one deterministic episode, the eval/stats.* means")
    args = ap.parse_args()
    if args.steps % SEQ:
        ap.error(f"--steps must be a multiple of the segment length {SEQ}")
    rank, world = 0, 1
    if args.learner and "WORLD_SIZE" in os.environ:              # one rank of a data-parallel run
        import torch.distributed as dist
        rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        if torch.cuda.is_available():
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
        dist.init_process_group(os.environ.get("HNS_DIST_BACKEND", "nccl" if torch.cuda.is_available() else "gloo"), rank=rank, world_size=world)
    offset, envs = sharding.env_shard(args.envs, world, rank)
    torch.manual_seed(0)
    if torch.cuda.is_available():
        from hns_amd import config
        from hns_amd.env import HideAndSeek
        env = HideAndSeek(config.make_cfg({"env": {"num_envs": envs}}, algo={"use_TP_net": 1}), env_index_offset=offset)
        env.set_seed(0)
        dev, A = env.device, env.num_agents
        D = env.observation_spec[("agents", "observation", "state_self")].shape[-1]
    else:
        env = StandInEnv(envs)
        env.set_seed(rank)
        dev, A, D = torch.device("cpu"), env.A, env.D
    actor, critic = Network(D, A, True, 0).to(dev), Network(D, A, False, 1).to(dev)
    pol = policy.RecurrentDevicePolicy(actor.names(), critic.names(), seed=rank)        # every rank samples its own noise
    col = collector.DeviceCollector(env, pol, args.steps, rnn_seq_len=SEQ)
    opt = torch.optim.Adam([*actor.parameters(), *critic.parameters()], lr=5e-4)
    vn = ValueNorm1().to(dev)
    huber = nn.HuberLoss(delta=10.0)
    steps_of = torch.arange(SEQ, device=dev)
    lrn = None
    if args.learner:
        cfg = {"ppo_epochs": args.updates, "num_minibatches": 4, "actor": {"rnn": {"train_seq_len": SEQ}}, "critic": {"rnn": {"train_seq_len": SEQ}}}
        if world > 1 or "WORLD_SIZE" in os.environ:
            lrn = DataParallelRecurrentLearner(actor.names(), critic.names(), cfg, tp_net=getattr(env, "TP", None), value_normalizer=vn, device_policy=pol,
                                               generator=torch.Generator(device=dev).manual_seed(rank), group="world")
        else:
            lrn = RecurrentDeviceLearner(actor.names(), critic.names(), cfg, tp_net=getattr(env, "TP", None), value_normalizer=vn, device_policy=pol)
    for it in range(2):
        st = col.collect()
        if lrn is not None:
            info = lrn.train_rollout(**st.learner_kwargs(), **st.recurrent_kwargs())
            if rank == 0:
                print(f"rollout {it}: " + "  ".join(f"{k.split('/')[-1]} {v:+.5f}" for k, v in info.items()))
            continue
        kw, rk = st.learner_kwargs(), st.recurrent_kwargs()
        N, T = kw["reward"].shape[:2]
        S = T // SEQ
        obs = (kw["obs_self"], kw.get("obs_others"), kw["obs_cylinders"])
        # the bootstrap value: one value_only call from the state and the flags going into the step after the last one
        next_value = pol.forward(*kw["next_obs_last"], critic_state=rk["last_critic_rnn_state"], is_init=rk["last_is_init"], value_only=True).value
        adv, returns, _ = gae.rollout_targets(kw["reward"], kw["done"].unsqueeze(-1), kw["state_value"], next_value, 0.995, 0.95, value_normalizer=vn)
        flat = lambda t: t.reshape(N * T, *t.shape[2:])
        adv, returns, old_v, old_lp, action = (flat(t) for t in (adv, returns, kw["state_value"], kw["log_probs"], kw["action"]))
        h0 = {n: rk[n].reshape(N * S, A, 128) for n in ("actor_rnn_state", "critic_rnn_state")}
        flags = rk["is_init"].reshape(N * S, 1, SEQ)            # the env-level flag of every step, per segment
        B = max(1, N * S // 4)
        for u in range(args.updates):
            seg = torch.randperm(N * S, device=dev)[:B]                                   # (env, segment) pairs: segment s of env n is n S + s
            index = (seg.unsqueeze(1) * SEQ + steps_of).reshape(B * SEQ)                    # their env-steps of the flattened [N T]
            loc = actor(obs, index, h0["actor_rnn_state"][seg].contiguous(), flags[seg], B, A)
            dist = torch.distributions.Normal(loc, torch.exp(actor.log_std))
            ratio = torch.exp(dist.log_prob(action[index]).sum(-1, keepdim=True) - old_lp[index])
            if it == 0 and u == 0:
                print(f"first minibatch, before any step: max |ratio - 1| = {float((ratio.detach() - 1).abs().max()):.3e}")
            a = adv[index]
            policy_loss = -torch.min(ratio * a, ratio.clamp(0.9, 1.1) * a).mean() - 1e-3 * dist.entropy().sum(-1).mean()
            values = critic(obs, index, h0["critic_rnn_state"][seg].contiguous(), flags[seg], B, A)
            b, r = old_v[index], returns[index]
            value_loss = torch.max(huber(r, values), huber(r, b + (values - b).clamp(-0.1, 0.1)))
            opt.zero_grad(set_to_none=True)
            (policy_loss + value_loss).backward()
            nn.utils.clip_grad_norm_([*actor.parameters(), *critic.parameters()], 10.0)
            opt.step()
            print(f"rollout {it} update {u}: policy loss {policy_loss.item():+.5f}  value loss {value_loss.item():.5f}  ({B} segments x {SEQ} steps x {A} agents)")
    if args.eval and rank == 0:
        for k, v in sorted(evaluator.DeviceEvaluator(env, pol, collector=col).evaluate(seed=0).items()):
            print(f"{k} = {v:.6g}")
    env.close()
    if lrn is not None and lrn.group is not None:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
