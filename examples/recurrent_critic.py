#!/usr/bin/env python3
"""A recurrent critic — the reference's `critic.rnn` configuration, which the fused update refuses — written in torch over hns_amd.encoder and
hns_amd.rnn:

    python examples/recurrent_critic.py --envs 256 --steps 32 --updates 8          # on the device: the rollout comes from DeviceCollector
    python examples/recurrent_critic.py --envs 4 --steps 32 --updates 2            # without a GPU: a seeded synthetic rollout, the torch restatements

The critic is an AttentionEncoder (HIP forward and backward under autograd), a GRU behind it (hns_gru_forward / hns_gru_backward: the
reference's GRUCell loop, is_init mask and LayerNorm(h + x) in one launch forward and three backward) and a torch nn.Linear(128, 1).  It is
trained on 16-step segments (the reference's train_seq_len) of the collected rollout: a minibatch is a set of (env, segment) pairs, the
encoder reads their env-steps in place through an index, the GRU reads the encoder's [B L A, 128] features in place as [B, A, L, 128], and
its dx is the encoder's d features.  is_init comes from the rollout's `done`: a step that follows a done step starts an episode.  The loss
is update_critic's clipped Huber loss; the step is clip_grad_norm_ + Adam in one launch (hns_adam_clipped through ClippedAdam).

The old values and the GAE targets (normalised by ValueNorm1, as the reference's) are the recurrent critic's own: one no_grad pass over all segments, and the one-step call (`[S, 128]`,
state in, state out — what collection runs per env step) on the rollout's last next observation for the bootstrap value.

What it leaves out (DESIGN-open-items.md, item 13): the rnn state at a segment's first step is not collected, so every segment starts from
zeros as an episode start does (is_init[:, 0] = 1)."""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hns_amd  # noqa: E402,F401
from hns_amd import critic_train, gae  # noqa: E402
from hns_amd.encoder import AttentionEncoder  # noqa: E402
from hns_amd.learner import ValueNorm1  # noqa: E402
from hns_amd.rnn import GRU  # noqa: E402

SEQ = 16                                                        # cfg/algo/mappo.yaml: train_seq_len


def device_rollout(envs, steps):
    from hns_amd import collector, config, policy
    from hns_amd.env import HideAndSeek
    env = HideAndSeek(config.make_cfg({"env": {"num_envs": envs}}, algo={"use_TP_net": 1}))
    env.set_seed(0)
    A = env.num_agents
    D = env.observation_spec[("agents", "observation", "state_self")].shape[-1]
    actor, critic = ({k: nn.Parameter(v.to(env.device)) for k, v in p.items()} for p in policy.random_parameters(D, A, seed=0))
    net = policy.DevicePolicy(actor, critic, seed=0)
    kw = collector.DeviceCollector(env, net, steps).collect().learner_kwargs()
    return kw, env


def synthetic_rollout(envs, steps, A=3, K=5, D=35):
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g)
    kw = {"obs_self": 0.7 * rn(envs, steps, A, 1, D), "obs_others": 0.5 * rn(envs, steps, A, A - 1, 3), "obs_cylinders": 0.5 * rn(envs, steps, A, K, 5),
          "reward": 0.1 * rn(envs, steps, A, 1), "done": torch.rand(envs, steps, 1, generator=g) < 0.05,
          "next_obs_last": (0.7 * rn(envs, A, 1, D), 0.5 * rn(envs, A, A - 1, 3), 0.5 * rn(envs, A, K, 5))}
    return kw, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--updates", type=int, default=8)
    args = ap.parse_args()
    if args.steps % SEQ:
        ap.error(f"--steps must be a multiple of the segment length {SEQ}")
    torch.manual_seed(0)
    kw, env = device_rollout(args.envs, args.steps) if torch.cuda.is_available() else synthetic_rollout(args.envs, args.steps)
    N, T, A = kw["reward"].shape[:3]
    D = kw["obs_self"].shape[-1]
    dev = kw["reward"].device
    # a step starts an episode when the step before it was done; a segment's first step starts from zeros (no collected rnn state)
    done = kw["done"].reshape(N, T).bool()
    is_init = torch.cat([torch.ones_like(done[:, :1]), done[:, :-1]], 1).reshape(N, T // SEQ, SEQ).clone()
    is_init[:, :, 0] = True

    encoder, rnn, head = AttentionEncoder(D, A).to(dev), GRU().to(dev), nn.Linear(128, 1).to(dev)
    nn.init.orthogonal_(head.weight, 0.01)                      # the reference's v_out: small first values, so the value clip (0.1) does not swallow the first steps
    nn.init.zeros_(head.bias)
    params = [*encoder.parameters(), *rnn.parameters(), *head.parameters()]
    opt = critic_train.ClippedAdam(params, lr=5e-4, max_grad_norm=10.0)
    loss_fn = nn.HuberLoss(delta=10.0)
    segments = N * (T // SEQ)
    B = max(1, segments // 4)
    steps_of = torch.arange(SEQ, device=dev)
    obs = (kw["obs_self"], kw.get("obs_others"), kw["obs_cylinders"])
    with torch.no_grad():                                       # collection's values: every segment in one call, then one step on the last next observation
        x = encoder(*obs).view(segments, SEQ, A, 128).transpose(1, 2)
        out, h = rnn(x, None, is_init.reshape(segments, 1, SEQ))
        old = head(out).transpose(1, 2).reshape(N, T, A, 1)
        h_end = h[:, :, 0].reshape(N, T // SEQ, A, 128)[:, -1].reshape(N * A, 128)
        x1 = encoder(*kw["next_obs_last"]).reshape(N * A, 128)
        o1, _ = rnn(x1, h_end, done[:, -1:].expand(N, A).reshape(N * A))
        next_value = head(o1).reshape(N, A, 1)
    # the reference's ValueNorm1: the critic works in normalised values, the targets are normalised by the returns' running moments
    _, returns, _ = gae.rollout_targets(kw["reward"], kw["done"].unsqueeze(-1), old, next_value, 0.995, 0.95, value_normalizer=ValueNorm1().to(dev))
    returns, old = returns.reshape(N * T, A, 1), old.reshape(N * T, A, 1)
    for u in range(args.updates):
        seg = torch.randperm(segments, device=dev)[:B]                                  # (env, segment) pairs: segment s of env n is seg = n (T / SEQ) + s
        index = (seg.unsqueeze(1) * SEQ + steps_of).reshape(B * SEQ)                      # their env-steps of the flattened [N T], segment-major
        feats = encoder(*obs, index, check_index=False)                                 # [B SEQ, A, 128], the rollout read in place
        x = feats.view(B, SEQ, A, 128).transpose(1, 2)                                  # [B, A, SEQ, 128]: a view, read in place
        out, _ = rnn(x, None, is_init.reshape(segments, 1, SEQ)[seg])                   # the env-level flag, [B, 1, SEQ]
        values = head(out).transpose(1, 2).reshape(B * SEQ, A, 1)
        b, r = old[index], returns[index]
        clipped = b + (values - b).clamp(-0.1, 0.1)
        loss = torch.max(loss_fn(r, values), loss_fn(r, clipped))
        for p in params:
            p.grad = None
        loss.backward()
        if dev.type == "cuda":
            opt.step(grad_norm=torch.linalg.vector_norm(torch.stack(torch._foreach_norm([p.grad for p in params]))))
        else:
            opt.step()
        print(f"update {u}: value loss {loss.item():.5f}  grad norm {float(opt.last_grad_norm):.4f}  ({B} segments x {SEQ} steps x {A} agents)")
    if env is not None:
        env.close()


if __name__ == "__main__":
    main()
