#!/usr/bin/env python3
"""What the recurrent device learner costs against what it replaces (profiles/r23_rnn_learner_cost.txt).

One process, alternating blocks after a warm-up, on a synthetic stored rollout at the reference default (2 048 envs x 64 steps x 3 agents,
train_seq_len 16, 16 minibatches: 512 segments = 24 576 rows a minibatch) and at 65 536 envs (16 384 segments = 786 432 rows):

    (a)  one minibatch pair (actor, then critic) through rnn_train.update_actor_rnn / update_critic_rnn
    (a') the same again: the spread between two arms that are the same code
    (b)  the pair as examples/recurrent_policy.py writes it: encoder.encode -> rnn.gru -> torch head, distribution, loss, clip_grad_norm_ and
         torch.optim.Adam — with two optimisers, one per network, so that the arithmetic matches (a)'s
    (c)  the reference's torch flow: the torch encoder, an nn.GRUCell stepped in a Python loop, LayerNorm(h + x), the same head / loss / clip / Adam
then a whole RecurrentDeviceLearner.train_rollout against (b) driven by hand over the same number of minibatches (bootstrap value and targets
included in both).  Times are wall clock around a block with a device synchronisation at both ends: the host's share counts.

    python tools/rnn_learner_cost.py [--envs 2048 65536] [--rounds 5] [--pairs 8]
    python tools/rnn_learner_cost.py --trace          # a few (a) pairs at both sizes and nothing else: run under a kernel trace
    python tools/rnn_learner_cost.py --group [--per-agent] [--envs 2048] [--rounds 5]

--group (profiles/r24_dp_rnn_learner_cost.txt): one train_rollout with the predictor on (4 epochs x 16 minibatches) through
RecurrentDeviceLearner without a group against DataParallelRecurrentLearner over a ONE-rank gloo group (a file store in a temporary directory),
in alternating blocks of this one process, and the same group-less learner a second time: the spread.  The difference is the data-parallel
path's cost with nobody to talk to — the global entries, the three collectives per minibatch pair, which gloo runs on host copies (a device
synchronisation each): an upper bound of the path's host cost under gloo, not an RCCL figure.  --per-agent: the same three arms with one
actor and one actor GRU per agent (profiles/r30_dp_per_agent_cost.txt): PerAgentRecurrentDeviceLearner against
DataParallelPerAgentRecurrentLearner."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hns_amd  # noqa: E402,F401
from hns_amd import gae, learner, rnn_train  # noqa: E402
from hns_amd import policy as P  # noqa: E402
from hns_amd import policy_train as PT  # noqa: E402
from hns_amd.encoder import AttentionEncoder  # noqa: E402
from hns_amd.rnn import GRU  # noqa: E402

L, T, A, K, D, M = 16, 64, 3, 5, 35, 16
DEV = "cuda" if torch.cuda.is_available() else "cpu"          # (the CPU: a functional check of the script at a toy size, not a measurement)


def sync():
    if DEV == "cuda":
        torch.cuda.synchronize()


class Network(nn.Module):
    """examples/recurrent_policy.py's network: encoder -> GRU -> head.  flow "ops": the HIP ops under autograd; "torch": the reference's
    torch statements (the torch encoder, an nn.GRUCell loop)."""

    def __init__(self, actor, seed):
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

    def forward(self, obs, index, h0, flags, B, flow):
        if flow == "ops":
            x = self.encoder(*obs, index, check_index=False).view(B, L, A, 128).transpose(1, 2)
            out, _ = self.rnn(x, h0, flags)
            return self.head(out).transpose(1, 2).reshape(B * L, A, -1)
        xs, xo, xc = obs
        N = xs.shape[0]
        g = lambda t: t.reshape(N * T, *t.shape[2:])[index]       # noqa: E731
        f = PT.encoder(self.encoder.parameters_by_field(), g(xs).unsqueeze(2), g(xo), g(xc)).view(B, L, A, 128)
        h, outs = h0, []
        keep = 1.0 - flags.reshape(B, 1, L).float()
        for t in range(L):
            h = h * keep[:, :, t:t + 1]
            h = self.rnn.cell(f[:, t].reshape(B * A, 128), h.reshape(B * A, 128)).view(B, A, 128)
            outs.append(h)
        y = self.rnn.layer_norm(torch.stack(outs, 1) + f)
        return self.head(y).reshape(B * L, A, -1)


def rollout(N, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)      # noqa: E731
    S = T // L
    return {"obs_self": 0.7 * rn(N, T, A, D), "obs_others": 0.5 * rn(N, T, A, A - 1, 3), "obs_cylinders": 0.5 * rn(N, T, A, K, 5),
            "action": rn(N, T, A, 4), "log_probs": -5.7 + 0.05 * rn(N, T, A, 1), "state_value": 0.1 * rn(N, T, A, 1),
            "next_obs_last": (0.7 * rn(N, A, D), 0.5 * rn(N, A, A - 1, 3), 0.5 * rn(N, A, K, 5)), "reward": 0.1 * rn(N, T, A, 1),
            "done": torch.rand(N, T, 1, device=DEV, generator=g) < 0.02}, \
           {"is_init": torch.rand(N, T, 1, device=DEV, generator=g) < 0.02, "actor_rnn_state": 0.5 * rn(N, S, A, 128), "critic_rnn_state": 0.5 * rn(N, S, A, 128),
            "rnn_seq_len": L, "last_critic_rnn_state": 0.5 * rn(N, A, 128), "last_is_init": torch.rand(N, 1, device=DEV, generator=g) < 0.02}


class TorchPair:
    """(b) / (c): one minibatch pair written in torch over a Network pair with two Adams."""

    def __init__(self, flow):
        self.flow = flow
        self.actor, self.critic = Network(True, 0).to(DEV), Network(False, 1).to(DEV)
        self.opts = [torch.optim.Adam(n.parameters(), lr=5e-4) for n in (self.actor, self.critic)]
        self.huber = nn.HuberLoss(delta=10.0)
        self.steps = torch.arange(L, device=DEV)

    def pair(self, kw, rk, adv, ret, seg):
        N = kw["obs_self"].shape[0]
        B, NS = seg.numel(), N * (T // L)
        obs = (kw["obs_self"], kw["obs_others"], kw["obs_cylinders"])
        index = (seg.unsqueeze(1) * L + self.steps).reshape(B * L)
        flags = rk["is_init"].reshape(NS, 1, L)[seg]
        flat = lambda t: t.reshape(N * T, *t.shape[2:])[index]    # noqa: E731
        loc = self.actor(obs, index, rk["actor_rnn_state"].reshape(NS, A, 128)[seg].contiguous(), flags, B, self.flow)
        dist = torch.distributions.Normal(loc, torch.exp(self.actor.log_std))
        ratio = torch.exp(dist.log_prob(flat(kw["action"])).sum(-1, keepdim=True) - flat(kw["log_probs"]))
        a = flat(adv)
        policy_loss = -torch.min(ratio * a, ratio.clamp(0.9, 1.1) * a).mean() * 4 - 1e-3 * dist.entropy().sum(-1).mean()
        self.opts[0].zero_grad(set_to_none=True)
        policy_loss.backward()
        nn.utils.clip_grad_norm_(self.actor.parameters(), 10.0)
        self.opts[0].step()
        values = self.critic(obs, index, rk["critic_rnn_state"].reshape(NS, A, 128)[seg].contiguous(), flags, B, self.flow)
        b, r = flat(kw["state_value"]), flat(ret)
        value_loss = torch.max(self.huber(r, values), self.huber(r, b + (values - b).clamp(-0.1, 0.1)))
        self.opts[1].zero_grad(set_to_none=True)
        value_loss.backward()
        nn.utils.clip_grad_norm_(self.critic.parameters(), 10.0)
        self.opts[1].step()


class DevicePair:
    """(a): the pair through update_actor_rnn / update_critic_rnn, workspaces kept, scalars into a table row."""

    def __init__(self):
        self.actor, self.critic = Network(True, 0).to(DEV), Network(False, 1).to(DEV)
        self.a, self.c = self.actor.names(), self.critic.names()
        self.opts = [rnn_train.make_optimizer(self.a, None, True), rnn_train.make_optimizer(self.c, None, False)]
        self.ws = [rnn_train.RnnWorkspace(), rnn_train.RnnWorkspace()]
        self.buckets = [rnn_train.make_bucket(self.a, True), rnn_train.make_bucket(self.c, False)] if DEV == "cuda" else [None, None]
        self.row = torch.empty(7, device=DEV)

    def pair(self, kw, rk, adv, ret, seg):
        obs = (kw["obs_self"], kw["obs_others"], kw["obs_cylinders"])
        rnn_train.update_actor_rnn(self.a, *obs, rk["actor_rnn_state"], rk["is_init"], kw["action"], kw["log_probs"], adv, self.opts[0], segment=seg,
                                   seq_len=L, workspace=self.ws[0], out=self.row[:4], bucket=self.buckets[0])
        rnn_train.update_critic_rnn(self.c, *obs, rk["critic_rnn_state"], rk["is_init"], kw["state_value"], ret, self.opts[1], segment=seg, seq_len=L,
                                    workspace=self.ws[1], out=self.row[4:], bucket=self.buckets[1])


def timed(fn, reps):
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps * 1e3


def report(name, xs):
    print(f"    {name:34s} median {statistics.median(xs):9.3f} ms   min {min(xs):9.3f}   max {max(xs):9.3f}   ({len(xs)} blocks)")
    return statistics.median(xs)


HIST, FUTURE = 10, 5                                            # the predictor's window and horizon (tests/rnn_update_reference.py's)


def group_cost(N, rounds, per_agent=False):
    import tempfile

    import torch.distributed as dist

    from hns_amd.tp_net import TPNet
    kw, rk = rollout(N)
    g = torch.Generator(device=DEV).manual_seed(3)
    kw["tp"] = (0.5 * torch.randn(N, T, HIST, 7 + 3 * A, device=DEV, generator=g), torch.rand(N, T, 3, device=DEV, generator=g) * 2 - 1,
                torch.ones(N, T, 1, device=DEV))
    cfg = {"ppo_epochs": 4, "num_minibatches": M, "TP_epochs": 1, "use_TP_net": 1, "actor": {"rnn": {"train_seq_len": L}}, "critic": {"rnn": {"train_seq_len": L}}}
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", rank=0, world_size=1, store=dist.FileStore(os.path.join(tmp, "store"), 1))

        if per_agent:
            cfg["share_actor"] = False
        local, dp = (learner.PerAgentRecurrentDeviceLearner, learner.DataParallelPerAgentRecurrentLearner) if per_agent else \
            (learner.RecurrentDeviceLearner, learner.DataParallelRecurrentLearner)

        def make(cls, **more):
            nets = Network(True, 0).to(DEV), Network(False, 1).to(DEV)
            actor = nets[0].names()
            if per_agent:                                        # A independently initialised actors, stacked
                each = [actor] + [Network(True, 10 + a).to(DEV).names() for a in range(1, A)]
                actor = {k: torch.stack([e[k].detach() for e in each]).contiguous() for k in actor}
            torch.manual_seed(5)
            return cls(actor, nets[1].names(), cfg, tp_net=TPNet(7 + 3 * A, 3 * FUTURE, FUTURE, 1).to(DEV),
                       value_normalizer=learner.ValueNorm1().to(DEV), generator=torch.Generator(device=DEV).manual_seed(2), **more)
        arms = {"group=None": make(local), "group=None again": make(local), "one-rank gloo group": make(dp, group="world")}
        times = {k: [] for k in arms}
        for arm in arms.values():
            arm.train_rollout(**kw, **rk)
        for _ in range(rounds):
            for k, arm in arms.items():
                times[k].append(timed(lambda: arm.train_rollout(**kw, **rk), 1))
        print(f"{local.__name__} / {dp.__name__}, {N} envs x {T} steps x {A} agents, L = {L}, predictor on: one train_rollout (4 epochs x {M} minibatches = {4 * M} pairs)")
        med = {k: report(k, v) for k, v in times.items()}
        extra = med["one-rank gloo group"] - med["group=None"]
        print(f"    spread group=None against itself: {abs(med['group=None'] - med['group=None again']):.3f} ms; the group's cost: {extra:.3f} ms a rollout, "
              f"{extra / (4 * M):.4f} ms a minibatch pair")
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[2048, 65536])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=8, help="minibatch pairs per timed block")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--skip-reference", action="store_true", help="leave (c) out (it is the slowest arm by far at 65 536 envs)")
    ap.add_argument("--group", action="store_true", help="a one-rank gloo group against group=None, whole rollouts, predictor on")
    ap.add_argument("--per-agent", action="store_true", help="with --group: one actor per agent (share_actor: False)")
    args = ap.parse_args()
    if args.group:
        for N in args.envs if args.envs != [2048, 65536] else [2048]:
            group_cost(N, args.rounds, args.per_agent)
        return
    for N in args.envs:
        kw, rk = rollout(N)
        NS = N * (T // L)
        B = NS // M
        gen = torch.Generator(device=DEV).manual_seed(1)
        segs = torch.randperm(NS, device=DEV, generator=gen).reshape(M, -1)
        adv, ret = torch.randn(N, T, A, 1, device=DEV, generator=gen), torch.randn(N, T, A, 1, device=DEV, generator=gen)
        print(f"{N} envs x {T} steps x {A} agents, L = {L}: {NS} segments, {M} minibatches of {B} segments = {B * L * A} rows")
        arms = {"(a)  update_*_rnn": DevicePair(), "(a') update_*_rnn again": DevicePair()}
        if args.trace:
            arm = arms["(a)  update_*_rnn"]
            for i in range(4):
                arm.pair(kw, rk, adv, ret, segs[i % M])
            sync()
            continue
        arms["(b)  encode -> gru -> torch head"] = TorchPair("ops")
        if not args.skip_reference:
            arms["(c)  torch encoder, GRUCell loop"] = TorchPair("torch")
        times = {k: [] for k in arms}
        for k, arm in arms.items():                              # warm-up: allocations, the first launches
            for i in range(2):
                arm.pair(kw, rk, adv, ret, segs[i])
        for r in range(args.rounds):
            for k, arm in arms.items():
                it = iter(range(10 ** 9))
                times[k].append(timed(lambda: arm.pair(kw, rk, adv, ret, segs[next(it) % M]), args.pairs))
        print("  one minibatch pair (actor + critic):")
        med = {k: report(k, v) for k, v in times.items()}
        ka, kb = list(arms)[:2]
        spread = abs(med[ka] - med[kb])
        print(f"    spread (a) against (a'): {spread:.3f} ms; (b) - (a) = {med[list(arms)[2]] - med[ka]:.3f} ms")
        # the whole rollout: train_rollout against (b) by hand over the same number of minibatches
        cfg = {"ppo_epochs": 4, "num_minibatches": M, "actor": {"rnn": {"train_seq_len": L}}, "critic": {"rnn": {"train_seq_len": L}}}
        nets = Network(True, 0).to(DEV), Network(False, 1).to(DEV)
        lrn = learner.RecurrentDeviceLearner(nets[0].names(), nets[1].names(), cfg, value_normalizer=learner.ValueNorm1().to(DEV),
                                             generator=torch.Generator(device=DEV).manual_seed(2))
        hand = TorchPair("ops")
        hp = P.RecurrentDevicePolicy(hand.actor.names(), hand.critic.names())
        vn = learner.ValueNorm1().to(DEV)

        def by_hand():
            nv = hp.forward(*kw["next_obs_last"], critic_state=rk["last_critic_rnn_state"], is_init=rk["last_is_init"], value_only=True).value
            a2, r2, _ = gae.rollout_targets(kw["reward"], kw["done"].unsqueeze(-1), kw["state_value"], nv, 0.995, 0.95, value_normalizer=vn)
            for _ in range(4):
                for seg in torch.randperm(NS, device=DEV, generator=gen).reshape(M, -1):
                    hand.pair(kw, rk, a2, r2, seg)

        whole = {"train_rollout": [], "(b) by hand, 64 pairs": []}
        lrn.train_rollout(**kw, **rk)
        by_hand()
        for r in range(max(2, args.rounds // 2)):
            whole["train_rollout"].append(timed(lambda: lrn.train_rollout(**kw, **rk), 1))
            whole["(b) by hand, 64 pairs"].append(timed(by_hand, 1))
        print("  one rollout (bootstrap value, targets, 4 epochs x 16 minibatches):")
        w = {k: report(k, v) for k, v in whole.items()}
        print(f"    by hand - train_rollout = {w['(b) by hand, 64 pairs'] - w['train_rollout']:.3f} ms (64 x the pair's spread: {64 * spread:.3f} ms)")
        del kw, rk, arms, lrn, hand, nets
        if DEV == "cuda":
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
