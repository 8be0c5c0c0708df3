#!/usr/bin/env python3
"""Generate tests/golden/g_gae.npz by EXECUTING the reference's rollout boundary (authoring container only: needs the reference checkout;
never run on the GPU box, never from tests).  Reuses make_golden.py's loaders without changing that file.

  gae cases   the reference's `compute_gae` and `compute_gae_` (learning/utils/gae.py:27-75, loaded by path) on [E, T, K] / [T, E, K] inputs:
              T in {1, 8, 64}, K in {1, 3, 7}, E <= 64; dones at t = 0, mid-rollout, t = T-1 and everywhere, bool [E, T, Kd] with Kd = 1
              (broadcast) or K; both (gamma, lambda) pairs (0.99 / 0.95, the functions' defaults; 0.995 / 0.95, cfg/algo/mappo.yaml); a forced
              -0.0 delta at the first step of the scan (env 4, k 0); and the same inputs through ValueNorm1.denormalize (valuenorm.py:100-104)
              first, with the normaliser's (sqrt(var), mean) stored
  train_op    MAPPOPolicy.train_op's block from the rewards to the normalised returns (learning/mappo.py:369-402, `_get_dones` :352-359), exec'd
              as written with a ValueNorm1 built from cfg/algo/mappo.yaml: three consecutive rollouts through one normaliser, E = 16, T = 64,
              A = 3 (rollout 1 with a two-column reward, summed by :370-371)
"""
import os
import sys
import types

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as M  # noqa: E402

MAPPO = "omni_drones/learning/mappo.py"
PAIRS = ((0.99, 0.95), (0.995, 0.95))
CASES = [(1, 1, 64, 1), (1, 3, 64, 3), (1, 7, 64, 1), (8, 1, 32, 1), (8, 3, 32, 3), (8, 7, 32, 1), (64, 1, 16, 1), (64, 3, 12, 3), (64, 7, 8, 1)]   # (T, K, E, Kd)


def _dones(g, E, T, Kd):
    d = torch.rand(E, T, Kd, generator=g) < 0.05
    d[0, :, :] = False
    d[0, 0, :] = True                       # t = 0
    d[1, :, :] = False
    d[1, T // 2, :] = True                  # mid-rollout
    d[2, :, :] = False
    d[2, T - 1, :] = True                   # t = T-1
    d[3, :, :] = True                       # every step
    d[4, T - 1, :] = True                   # (the -0.0 delta below)
    return d


def gen_gae_cases(out, ref, vn_cls, beta, seed=20261015):
    g = torch.Generator().manual_seed(seed)
    vn = vn_cls(input_shape=(1,), beta=beta)
    for _ in range(3):
        vn.update(torch.randn(64, 1, generator=g) * 3.0 + 7.0)
    mean, var = vn.running_mean_var()
    out["dn_scale"], out["dn_shift"] = torch.sqrt(var), mean
    for T, K, E, Kd in CASES:
        cid = f"t{T}k{K}"
        reward = torch.randn(E, T, K, generator=g) * 0.5
        value = torch.randn(E, T, K, generator=g) * 2.0
        next_value = torch.randn(E, K, generator=g) * 2.0
        done = _dones(g, E, T, Kd)
        # env 4, k 0, t = T-1: r = -0.0, nv < 0 with done (gamma * nv * 0 = -0.0), v = +0.0 -> delta = -0.0; the reference's `gae = 0` makes it +0.0
        reward[4, T - 1, 0], value[4, T - 1, 0], next_value[4, 0] = -0.0, 0.0, -1.5
        nd = 1.0 - done.float()
        delta = reward[4, T - 1, 0] + 0.99 * next_value[4, 0] * nd[4, T - 1, 0] - value[4, T - 1, 0]
        assert float(delta) == 0.0 and torch.signbit(delta)
        out[f"{cid}_reward"], out[f"{cid}_value"], out[f"{cid}_done"], out[f"{cid}_next_value"] = reward, value, done, next_value
        tm = lambda x: x.transpose(0, 1).contiguous()          # noqa: E731
        for gi, (gamma, lmbda) in enumerate(PAIRS):
            adv, ret = ref.compute_gae(reward, done, value, next_value, gamma=gamma, lmbda=lmbda)
            adv_, ret_ = ref.compute_gae_(tm(reward), tm(done), tm(value), next_value, gamma=gamma, lmbda=lmbda)
            assert torch.equal(tm(adv), adv_) and torch.equal(tm(ret), ret_)
            assert not torch.signbit(adv[4, T - 1, 0])
            out[f"{cid}_g{gi}_adv"], out[f"{cid}_g{gi}_ret"] = adv, ret
            out[f"{cid}_g{gi}_adv_tm"], out[f"{cid}_g{gi}_ret_tm"] = adv_, ret_
        # mappo.py:377-379 in front of the same GAE: every value read through ValueNorm1.denormalize
        gamma, lmbda = PAIRS[1]
        adv, ret = ref.compute_gae(reward, done, vn.denormalize(value.unsqueeze(-1)).squeeze(-1), vn.denormalize(next_value.unsqueeze(-1)).squeeze(-1),
                                   gamma=gamma, lmbda=lmbda)
        out[f"{cid}_dn_adv"], out[f"{cid}_dn_ret"] = adv, ret
    out["pairs"] = np.array(PAIRS, dtype=np.float64)
    out["cases"] = np.array(CASES, dtype=np.int64)


def gen_train_op(out, ref, vn_cls, algo, E=16, T=64, A=3, rollouts=3, seed=20261016):
    stmts = M._stmt_sources(MAPPO, "MAPPOPolicy", "train_op", lambda s: True)
    first = next(i for i, s in enumerate(stmts) if s.startswith("rewards = tensordict.get("))
    last = next(i for i, s in enumerate(stmts) if s.startswith("if hasattr(self, \"value_normalizer\")") and "value_normalizer.update" in s)
    blocks = stmts[first:last + 1]
    assert any("compute_gae(" in b for b in blocks) and any("denormalize" in b for b in blocks), blocks
    get_dones = M.exec_functions(M.extract_source(MAPPO, ["_get_dones"], "MAPPOPolicy"), {"torch": torch, "TensorDict": dict})["_get_dones"]
    vcfg = algo["critic"]["value_norm"]
    assert vcfg["class"] == "ValueNorm1" and algo["normalize_advantages"] is True
    self = types.SimpleNamespace(normalize_advantages=algo["normalize_advantages"], gae_gamma=algo["gamma"], gae_lambda=algo["gae_lambda"],
                                 reward_name=("agents", "reward"), agent_spec=types.SimpleNamespace(name="agents", n=A),
                                 value_normalizer=vn_cls(input_shape=(1,), **vcfg["kwargs"]))
    self._get_dones = lambda td: get_dones(self, td)
    g = torch.Generator().manual_seed(seed)
    for r in range(rollouts):
        R = 2 if r == 1 else 1
        reward = torch.randn(E, T, A, R, generator=g) * 0.4 + 0.1 * r
        value = torch.randn(E, T, A, 1, generator=g) * (1.0 + r)          # critic output (normalised space)
        next_value = torch.randn(E, A, 1, generator=g) * (1.0 + r)
        env_done = torch.rand(E, T, 1, generator=g) < 0.03
        env_done[0, T - 1], env_done[1, 0], env_done[2, T // 2] = True, True, True
        tensordict = {("next", "agents", "reward"): reward.clone(), "state_value": value.clone(), ("next", "done"): env_done.clone()}
        ns = {"self": self, "tensordict": tensordict, "torch": torch, "compute_gae": ref.compute_gae,
              "value_output": {"state_value": next_value.clone()}}
        for code in blocks:
            exec(code, ns)
        vn = self.value_normalizer
        p = f"r{r}_"
        out[p + "reward"], out[p + "value"], out[p + "next_value"], out[p + "env_done"] = reward, value, next_value, env_done
        out[p + "dones"] = ns["dones"]
        out[p + "adv_normalised"], out[p + "ret_normalised"] = tensordict["advantages"], tensordict["returns"]
        out[p + "running_mean"], out[p + "running_mean_sq"] = vn.running_mean.clone(), vn.running_mean_sq.clone()
        out[p + "debiasing_term"] = vn.debiasing_term.clone()
    out["train_meta"] = np.array([E, T, A, rollouts], dtype=np.int64)
    out["train_gamma_lambda"] = np.array([algo["gamma"], algo["gae_lambda"]], dtype=np.float64)
    out["beta"] = np.float64(vcfg["kwargs"]["beta"])


def main():
    torch.set_num_threads(1)
    ref = M.load_by_path("ref_gae", "omni_drones/learning/utils/gae.py")
    valuenorm = M.load_by_path("ref_valuenorm", "omni_drones/learning/utils/valuenorm.py")
    algo = yaml.safe_load(open(os.path.join(M.REF, "cfg/algo/mappo.yaml")))
    assert (algo["gamma"], algo["gae_lambda"]) == PAIRS[1]
    vn_cls = getattr(valuenorm, algo["critic"]["value_norm"]["class"])
    out = {}
    gen_gae_cases(out, ref, vn_cls, algo["critic"]["value_norm"]["kwargs"]["beta"])
    gen_train_op(out, ref, vn_cls, algo)
    M.save("g_gae", **out)


if __name__ == "__main__":
    main()
