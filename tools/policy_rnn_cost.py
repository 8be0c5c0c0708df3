#!/usr/bin/env python3
"""Cost of the fused recurrent policy step (hns_policy_forward_rnn through hns_amd.policy.RecurrentDevicePolicy) on the GPU, in one process, in
alternating blocks, medians and the block-to-block spread, at 2 048 and 65 536 envs (3 pursuers, 5 cylinders, state_self 35):

  fused     : RecurrentDevicePolicy.forward — ONE launch (and the counter bump): encoder -> GRU step -> head for both networks, states in place
  (a) ops   : what a user wrote before it: encoder.encode -> rnn.gru one-step, per network, then torch heads, torch.randn sampling and
              Normal.log_prob; the states carried
  (b) torch : the reference's statements in torch on the same GPU (policy.torch_forward_rnn: F.multi_head_attention_forward, the GRUCell
              statements, F.layer_norm)
  (c) floor : the non-recurrent DevicePolicy.forward (hns_policy_forward) on the same encoder and head parameters

and one collector step (DeviceCollector.collect() over 16 steps / 16), recurrent against non-recurrent, on HideAndSeek.

usage  python tools/policy_rnn_cost.py [--blocks 7] [--window 0.25] [--envs 2048,65536] [--only fused] [--no-collector]
`--only fused` runs the fused path alone: the run to put under `rocprofv3 --kernel-trace --stats -- python tools/policy_rnn_cost.py --only
fused --no-collector` for the kernel's own time.  A path's repetitions per block fill `--window` seconds (calibrated once)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import hns_amd  # noqa: E402,F401
from hns_amd import collector, config, encoder, rnn  # noqa: E402
from hns_amd import policy as P  # noqa: E402

A, K, D = 3, 5, 35


def network(dev, D=D):
    actor, critic = P.random_parameters(D, A, seed=0)
    for k, p in enumerate((actor, critic)):
        p.update(P.random_rnn_parameters(seed=1 + k))
    return {k: v.to(dev) for k, v in actor.items()}, {k: v.to(dev) for k, v in critic.items()}


def blocks(paths, nblocks, window):
    """{name: (median ms, [block ms])}: warm-up, a calibration of the repetitions, then alternating blocks."""
    reps = {}
    for k, fn in paths.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        reps[k] = max(5, int(window / max((time.perf_counter() - t0) / 5, 1e-6)))
    times = {k: [] for k in paths}
    for _ in range(nblocks):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[k]):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / reps[k] * 1e3)
    return {k: (sorted(t)[len(t) // 2], t) for k, t in times.items()}, reps


def report(res, reps, label):
    for k, (med, t) in res.items():
        print(f"  {label.get(k, k):<22}: median {med * 1e3:9.1f} us   spread {min(t) * 1e3:.1f}-{max(t) * 1e3:.1f}   ({reps[k]} calls per block; blocks "
              f"{' '.join(f'{v * 1e3:.1f}' for v in t)})")


def forward_paths(E, dev, only):
    actor, critic = network(dev)
    pol = P.RecurrentDevicePolicy(actor, critic, seed=0)
    plain = P.DevicePolicy(*({k: v for k, v in p.items() if not k.startswith("rnn.")} for p in (actor, critic)), seed=0)
    g = torch.Generator(device=dev).manual_seed(0)
    xs = 0.7 * torch.randn(E, A, 1, D, device=dev, generator=g)
    xo = 0.5 * torch.randn(E, A, A - 1, 3, device=dev, generator=g)
    xc = 0.5 * torch.randn(E, A, K, 5, device=dev, generator=g)
    st = {n: [0.5 * torch.randn(E, A, 128, device=dev, generator=g) for _ in range(2)] for n in ("fused", "ops", "torch")}
    enc = [{k: v for k, v in p.items() if k in encoder.FIELDS} for p in (pol.actor_p, pol.critic_p)]
    grus = [pol.actor_rnn, pol.critic_rnn]
    scale = torch.exp(pol.actor_p["log_std"])

    def fused():
        pol.forward(xs, xo, xc, actor_state=st["fused"][0], critic_state=st["fused"][1], out_states=st["fused"])

    def ops():
        with torch.no_grad():
            ys = []
            for k in range(2):
                f = encoder.encode(enc[k], xs, xo, xc).reshape(E * A, 128)
                y, h = rnn.gru(grus[k], f, st["ops"][k].view(E * A, 128))
                st["ops"][k] = h.view(E, A, 128)
                ys.append(y.view(E, A, 128))
            loc = F.linear(ys[0], pol.actor_p["head_w"], pol.actor_p["head_b"])
            action = loc + scale * torch.randn_like(loc)
            logp = torch.distributions.Normal(loc, scale).log_prob(action).sum(-1, keepdim=True)
            value = F.linear(ys[1], pol.critic_p["head_w"], pol.critic_p["head_b"])
        return action, logp, value

    def ref():
        with torch.no_grad():
            out = P.torch_forward_rnn(pol.actor_p, pol.critic_p, pol.actor_rnn, pol.critic_rnn, xs, xo, xc, st["torch"][0], st["torch"][1])
        st["torch"] = [out.actor_state, out.critic_state]

    def floor():
        plain.forward(xs, xo, xc)

    paths = {"fused": fused, "ops": ops, "torch": ref, "floor": floor}
    return {only: paths[only]} if only else paths


def collector_paths(E, dev):
    from hns_amd.env import HideAndSeek
    T = 16
    out, envs = {}, []
    for name in ("recurrent", "plain"):
        env = HideAndSeek(config.make_cfg({"num_agents": A, "cylinder": {"max_num": K, "min_num": K}, "env": {"num_envs": E}}, algo={"use_TP_net": 1}),
                          headless=True)                        # with the trajectory predictor's rows: state_self 35, the flagship's
        env.set_seed(0)
        envs.append(env)
        actor, critic = network(dev, env.observation_spec[("agents", "observation", "state_self")].shape[-1])
        if name == "recurrent":
            col = collector.DeviceCollector(env, P.RecurrentDevicePolicy(actor, critic, seed=0), T, rnn_seq_len=T)
        else:
            col = collector.DeviceCollector(env, P.DevicePolicy(*({k: v for k, v in p.items() if not k.startswith("rnn.")} for p in (actor, critic)),
                                                                  seed=0), T)
        out[name] = col.collect
    return out, envs, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--envs", default="2048,65536")
    ap.add_argument("--only", choices=("fused", "ops", "torch", "floor"), default=None)
    ap.add_argument("--no-collector", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("policy_rnn_cost: no GPU — nothing is measured without one")
    dev = torch.device("cuda")
    label = {"fused": "fused (one launch)", "ops": "(a) encode, gru, heads", "torch": "(b) torch statements", "floor": "(c) non-recurrent"}
    for E in (int(v) for v in a.envs.split(",")):
        print(f"policy step, {E} envs x {A} agents = {E * A} rows, K {K}, D {D}: sampling forward pass, both networks, states carried")
        res, reps = blocks(forward_paths(E, dev, a.only), a.blocks, a.window)
        report(res, reps, label)
        if not a.only:
            f, o = res["fused"], res["ops"]
            spread = max(max(f[1]) - min(f[1]), max(o[1]) - min(o[1]))
            verdict = "BELOW (a) by more than the spread" if o[0] - f[0] > spread else "NOT below (a) by more than the spread"
            print(f"  fused / (a) {f[0] / o[0]:.2f}, fused / (c) {f[0] / res['floor'][0]:.2f}, (b) / fused {res['torch'][0] / f[0]:.1f}; (a) - fused "
                  f"{(o[0] - f[0]) * 1e3:.1f} us against a block-to-block spread of {spread * 1e3:.1f} us: fused is {verdict}")
        torch.cuda.empty_cache()
        if not a.no_collector and not a.only:
            paths, envs, T = collector_paths(E, dev)
            res, reps = blocks(paths, a.blocks, a.window)
            print(f"collector, {E} envs: one collect() of {T} steps (policy, two fused stores, env step; recurrent: + the segment store)")
            for k, (med, t) in res.items():
                print(f"  {k:<10}: median {med / T * 1e3:9.1f} us per step   spread {min(t) / T * 1e3:.1f}-{max(t) / T * 1e3:.1f}   ({reps[k]} collects per block)")
            print(f"  recurrent - plain: {(res['recurrent'][0] - res['plain'][0]) / T * 1e3:.1f} us per step")
            for env in envs:
                env.close()
            del paths
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
