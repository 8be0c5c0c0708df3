#!/usr/bin/env python3
"""Cost of the rollout boundary on the device: hns_gae + hns_rollout_normalise against the reference's torch statements (learning/mappo.py:370-402:
ValueNorm1.denormalize, compute_gae's loop over T, the advantage mean / std and normalisation, ValueNorm1.update / normalize), both on the GPU, in ONE
process, alternating timed blocks (hipEvent pairs around N back-to-back calls), at 2 048 and 65 536 envs x T 64 x 3 agents, batch-major
([N, T, A, 1], compute_gae) and time-major ([T, N, A, 1], compute_gae_).

    python tools/gae_cost.py [--blocks 7 --reps 20]      -> profiles/r07_gae_cost.txt
    python tools/gae_cost.py --profile                  (a short run of the two library calls only, for rocprofv3 --kernel-trace --stats)

Bytes are what the algorithm must move: GAE + moments reads reward, value (4 B), done (1 B per env and step) and next_value and writes advantages
and returns (4 B); the normalisation reads and writes both arrays once.  The fraction is bytes / time over 8 TB/s (the HBM peak)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hns_amd  # noqa: E402,F401
from hns_amd import gae, sharding  # noqa: E402

PEAK = 8e12
A, T = 3, 64
GAMMA, LMBDA = 0.995, 0.95


class VN:
    """ValueNorm1's state (learning/utils/valuenorm.py:45-106), on the device."""

    def __init__(self, dev):
        self.beta, self.epsilon = 0.995, 1e-5
        self.running_mean = torch.full((1,), 0.03, device=dev)
        self.running_mean_sq = torch.full((1,), 0.2, device=dev)
        self.debiasing_term = torch.tensor(0.05, device=dev)

    def running_mean_var(self):
        d = self.debiasing_term.clamp(min=self.epsilon)
        mean, mean_sq = self.running_mean / d, self.running_mean_sq / d
        return mean, (mean_sq - mean ** 2).clamp(min=1e-2)

    def update(self, x):                       # valuenorm.py:83-91
        batch_mean, batch_sq_mean = x.mean(dim=tuple(range(x.dim() - 1))), (x ** 2).mean(dim=tuple(range(x.dim() - 1)))
        self.running_mean.mul_(self.beta).add_(batch_mean * (1.0 - self.beta))
        self.running_mean_sq.mul_(self.beta).add_(batch_sq_mean * (1.0 - self.beta))
        self.debiasing_term.mul_(self.beta).add_(1.0 * (1.0 - self.beta))


def torch_boundary(reward, done, value, next_value, vn, tm):
    """mappo.py:377-402 as torch launches (the reference's loop: gae.py:27-75)."""
    mean, var = vn.running_mean_var()
    values = value * torch.sqrt(var) + mean
    nv = next_value * torch.sqrt(var) + mean
    adv, ret = gae._torch_gae(reward, done, values, nv, GAMMA, LMBDA, tm)
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    vn.update(ret)
    mean, var = vn.running_mean_var()
    ret = (ret - mean) / torch.sqrt(var)
    return adv, ret


def hns_boundary(reward, done, value, next_value, scale, shift, sc, tm, m_a, d_a, m_r, s_r):
    """The two library calls: hns_gae (GAE + moment row: two launches) and hns_rollout_normalise (one launch); the scalars between them are taken
    as given (in rollout_targets torch forms them from the gathered table: a handful of one-element launches, timed separately below)."""
    adv, ret, row = gae._launch_gae(reward, done, value, next_value, GAMMA, LMBDA, tm, scale, shift, sc, moments=True)
    gae.rollout_normalise(adv, ret, m_a, d_a, m_r, s_r)
    return adv, ret, row


def inputs(E, tm, dev):
    g = torch.Generator(device=dev).manual_seed(E)
    shape = (T, E, A, 1) if tm else (E, T, A, 1)
    reward = torch.randn(*shape, device=dev, generator=g) * 0.4
    value = torch.randn(*shape, device=dev, generator=g)
    done = torch.rand(*shape[:2], 1, 1, device=dev, generator=g) < 0.02
    next_value = torch.randn(E, A, 1, device=dev, generator=g)
    success = (torch.rand(E, device=dev, generator=g) < 0.3).float()
    return reward, done, value, next_value, success


def time_calls(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / reps        # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gae_cost.py measures on the GPU; no device here")
    dev = torch.device("cuda")
    print(f"# {torch.cuda.get_device_name(0)}; T {T} x A {A}; gamma {GAMMA} lambda {LMBDA}; {args.blocks} alternating blocks x {args.reps} calls; "
          f"us per call: median [min, max] over blocks")
    for E in (2048, 65536):
        for tm in (False, True):
            reward, done, value, nv, success = inputs(E, tm, dev)
            vn = VN(dev)
            mean, var = vn.running_mean_var()
            scale, shift = torch.sqrt(var), mean
            m_a, d_a, m_r, s_r = (torch.full((1,), x, device=dev) for x in (0.1, 1.7, -0.2, 2.5))
            n = reward.numel()
            gae_bytes = 16 * n + done.numel() + 4 * nv.numel() + 4 * success.numel()
            norm_bytes = 16 * n
            hns = lambda: hns_boundary(reward, done, value, nv, scale, shift, success, tm, m_a, d_a, m_r, s_r)   # noqa: E731
            if args.profile:
                for _ in range(args.reps):
                    hns()
                torch.cuda.synchronize()
                continue
            gae_only = lambda: gae._launch_gae(reward, done, value, nv, GAMMA, LMBDA, tm, scale, shift, success, moments=True)   # noqa: E731
            adv, ret, _ = gae_only()
            norm_only = lambda: gae.rollout_normalise(adv, ret, m_a, d_a, m_r, s_r)   # noqa: E731
            full = lambda: gae.rollout_targets(reward, done, value, nv, GAMMA, LMBDA, value_normalizer=vn, success=success, time_major=tm)  # noqa: E731
            ref = lambda: torch_boundary(reward, done, value, nv, vn, tm)   # noqa: E731
            arms = {"hns_gae (GAE + moments)": gae_only, "hns_rollout_normalise": norm_only, "both library calls": hns,
                    "rollout_targets (whole)": full, "torch statements (reference)": ref}
            for f in arms.values():                                   # warm-up every shape
                f()
            torch.cuda.synchronize()
            res = {k: [] for k in arms}
            for _ in range(args.blocks):
                for k, f in arms.items():
                    res[k].append(time_calls(f, args.reps))
            lay = "time-major [T,N,A,1]" if tm else "batch-major [N,T,A,1]"
            print(f"\n{E} envs, {lay}: {n} values; GAE + moments {gae_bytes / 1e6:.1f} MB, normalisation {norm_bytes / 1e6:.1f} MB")
            for k, v in res.items():
                v = sorted(v)
                med = v[len(v) // 2]
                extra = ""
                if k.startswith("hns_gae"):
                    extra = f"  {gae_bytes / med / 1e6:7.2f} TB/s = {gae_bytes / med / 1e-6 / PEAK:.2f} of 8 TB/s"
                elif k.startswith("hns_rollout"):
                    extra = f"  {norm_bytes / med / 1e6:7.2f} TB/s = {norm_bytes / med / 1e-6 / PEAK:.2f} of 8 TB/s"
                print(f"  {k:32s} {med:10.1f} us  [{v[0]:.1f}, {v[-1]:.1f}]{extra}")
            print(f"  torch / both library calls: {sorted(res['torch statements (reference)'])[args.blocks // 2] / sorted(res['both library calls'])[args.blocks // 2]:.1f}x")


if __name__ == "__main__":
    main()
