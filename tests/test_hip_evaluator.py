"""Device evaluation on the GPU: hns_policy_act, hns_eval_means, DeviceEvaluator and the training example's evaluation / checkpoint flags.

hns_policy_act: `action` is bit for bit hns_policy_forward's with HNS_POLICY_DETERMINISTIC at policy_reference.py's edge shapes (D 1 / 35 /
96; 1, 31, 32, 33 and more rows around the 32-row tile; A = 1 without state_others and A = 3; K 1 / 16; sliced observations; through out=),
and the call writes nothing but `action`, reads neither the critic image nor the call counter.  hns_eval_means: against math.fsum within the
derived bound of eval_cases.py, `used` exact, guard words, two calls bit-identical.  DeviceEvaluator: `stats` equals the statistics a hand
loop (forward(deterministic=True) -> step) holds after the last step and the reference's take_first_episode over that loop's stacked ones;
an evaluation between two training iterations leaves every info row, parameter, optimiser and ValueNorm tensor bit for bit what it is
without it.  examples/train_device.py: evaluates, writes its checkpoints and resumes from one, in child processes."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_cases as EC
import learner_cases as LC
import policy_reference as R
from hns_amd import abi, collector, config, evaluator, learner
from hns_amd import policy as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------------------------------
# hns_policy_act
# (A, K, D, E): E A = 1, 31, 32, 33 rows around the 32-row tile and 63, 120 rows in several tiles; D 1, 35, 96; K 1, 16; A = 1 and 3
ACT_SHAPES = [(1, 1, 1, 1), (1, 16, 35, 31), (1, 5, 96, 32), (1, 5, 35, 33), (3, 5, 35, 11), (3, 16, 96, 21), (3, 1, 1, 1), (3, 5, 35, 40)]


def _policy(A, D, seed):
    actor, critic = R.random_net(D, A, seed)
    t = lambda p: {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}          # noqa: E731
    return P.DevicePolicy(t(actor), t(critic), seed=seed)


def _obs(E, A, K, D, seed, sliced=False):
    """(state_self [E, A, D], state_others or None, cylinders) on the device; sliced: views of larger tensors — a longer row, a skipped
    token, skipped envs — with the last axis's stride still 1 (what the entry point takes without a copy)."""
    if not sliced:
        obs, _ = R.random_obs(E, A, K, D, seed)
        g = lambda k: torch.from_numpy(obs[k]).to(DEV) if k in obs else None       # noqa: E731
        return g("state_self"), g("state_others"), g("cylinders")
    gen = torch.Generator().manual_seed(seed)
    xs = (torch.randn(E, A, 1, D + 3, generator=gen) * 0.7).to(DEV)[..., 2:D + 2]
    xo = (torch.randn(E, A, A, 3, generator=gen) * 0.5).to(DEV)[:, :, 1:] if A > 1 else None
    xc = (torch.randn(E + 2, A, K + 1, 5, generator=gen) * 0.5).to(DEV)[1:-1, :, :K]
    assert E * A == 1 or (not xs.is_contiguous() and not xc.is_contiguous())      # (one row of one token: any view of it is contiguous)
    return xs, xo, xc


@pytest.mark.parametrize("sliced", [False, True], ids=["contiguous", "sliced"])
@pytest.mark.parametrize("shape", ACT_SHAPES, ids=["a%dk%dd%de%d" % s for s in ACT_SHAPES])
def test_act_is_the_deterministic_forwards_action_bit_for_bit(shape, sliced):
    A, K, D, E = shape
    pol = _policy(A, D, 900 + 10 * A + K + D)
    xs, xo, xc = _obs(E, A, K, D, 17 + E, sliced)
    want = pol.forward(xs, xo, xc, deterministic=True).action
    got = pol.act(xs, xo, xc)
    assert got.shape == (E, A, 4) and torch.isfinite(got).all() and float(got.abs().max()) > 0
    assert LC.bits_equal(got, want)
    out = torch.full((E, A, 4), 7.0, device=DEV)
    assert pol.act(xs, xo, xc, out=out) is out and LC.bits_equal(out, want)


@pytest.mark.parametrize("shape", [(1, 5, 35, 33), (3, 5, 35, 11)], ids=["a1", "a3"])
def test_act_writes_only_the_action_and_reads_neither_the_critic_nor_the_counter(shape):
    A, K, D, E = shape
    rows = E * A
    pol = _policy(A, D, 5)
    xs, xo, xc = _obs(E, A, K, D, 6)
    want = pol.forward(xs, xo, xc, deterministic=True).action.clone()
    counter = pol.counter.clone()
    G = 64                                                       # guard words behind every output
    action = torch.full((rows * 4 + G,), -77.0, device=DEV)
    others = {k: torch.full((n + G,), v, device=DEV) for k, n, v in (("log_prob", rows, 11.0), ("value", rows, 12.0), ("loc", rows * 4, 13.0))}
    xs, xo, xc, io = pol._io(xs.squeeze(2), xo, xc)
    io.action = action.data_ptr()
    for k, t in others.items():
        setattr(io, k, t.data_ptr())
    lib = abi.load_library()
    # the critic half of the image is never read: NaN there must not reach the action
    img = pol.packed.view(torch.float32)
    img[img.numel() // 2:] = float("nan")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    abi.check(lib.hns_policy_act(pol.packed.data_ptr(), D, E, A, K, C.byref(io), st), "hns_policy_act")
    torch.cuda.synchronize()
    assert LC.bits_equal(action[:rows * 4].view(E, A, 4), want)
    assert bool((action[rows * 4:] == -77.0).all())
    for (k, t), v in zip(others.items(), (11.0, 12.0, 13.0)):
        assert bool((t == v).all()), f"{k} was written"
    assert torch.equal(pol.counter, counter)
    assert LC.bits_equal(pol.act(xs, xo, xc), want) and torch.equal(pol.counter, counter)        # ... and through the class


# ---------------------------------------------------------------------------------------------------------------------------------------
# hns_eval_means
def _means(table, stride, n, mask, guard=16):
    """hns_eval_means over table's rows (stride 1: table [count, n]; else table [n, count], a view whose rows are `stride` apart): (mean, used) with their guard words."""
    count = table.shape[1] if stride > 1 else table.shape[0]
    rows = (abi.HnsEvalRow * abi.HNS_EVAL_MAX_ROWS)()
    for i in range(count):
        rows[i].src, rows[i].stride = (table[:, i] if stride > 1 else table[i]).data_ptr(), stride
    mean = torch.full((count + guard,), -55.0, device=DEV)
    used = torch.full((count + 1 + guard,), -66, dtype=torch.int64, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    abi.check(abi.load_library().hns_eval_means(rows, count, n, mask.data_ptr() if mask is not None else None, mean.data_ptr(), used.data_ptr(), st),
              "hns_eval_means")
    torch.cuda.synchronize()
    return mean.cpu().numpy(), used.cpu().numpy()


@pytest.mark.parametrize("count", [1, 24, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_eval_means_against_fsum(n, count):
    host = EC.make_rows(count, n, seed=1000 * count + n)
    flat = torch.from_numpy(host).to(DEV)                                        # [count, n]: stride 1
    wide = torch.zeros(n, count + 2, device=DEV)                                 # [n, count + 2]: row i is column i + 1, stride count + 2
    wide[:, 1:count + 1] = flat.T
    for kind in (None, "partial", "zero"):
        m = EC.make_mask(kind, n, seed=n + count)
        mask = torch.from_numpy(m).to(DEV) if m is not None else None
        want_used = [EC.exact_mean(host[i], m)[2] for i in range(count)]
        ref_mean, ref_used, ref_masked = evaluator.stat_means(host, m)
        for table, stride in ((flat, 1), (wide[:, 1:count + 1], count + 2)):
            mean, used = _means(table, stride, n, mask)
            what = f"n {n}, {count} rows, mask {kind}, stride {stride}"
            assert (mean[count:] == -55.0).all() and (used[count + 1:] == -66).all(), what + ": guard words"
            for i in range(count):
                EC.check_mean(mean[i], host[i], m, f"{what}, row {i}")
            assert used[:count].tolist() == want_used and used[count] == (n if m is None else int((m != 0).sum())), what
            if kind == "zero":
                assert np.isnan(mean[:count]).all() and not used[:count + 1].any()
            again = _means(table, stride, n, mask)
            assert np.array_equal(mean.view(np.int32), again[0].view(np.int32)) and np.array_equal(used, again[1]), what + ": two calls differ"
            # the host restatement runs the kernel's order: the same bits
            assert np.array_equal(mean[:count], ref_mean, equal_nan=True) and np.array_equal(used[:count], ref_used), what
            assert used[count] == ref_masked


# ---------------------------------------------------------------------------------------------------------------------------------------
# DeviceEvaluator against the hand loop
def _make_env(task, use_tp, seed=0):
    from hns_amd.env import HideAndSeek
    torch.manual_seed(seed + 100)                                # the predictor's initial weights come from the global generator
    env = HideAndSeek(config.make_cfg(task, algo={"use_TP_net": int(use_tp)}), headless=True)
    env.set_seed(seed)
    return env


def _env_policy(env, seed):
    D = abi.self_dim(env.num_targets) + (3 * env.tp_future_step * env.num_targets if env.use_TP_net else 0)
    actor, critic = P.random_parameters(D, env.num_agents, seed=seed)
    actor["act_dist.fc_mean.weight"] = actor["act_dist.fc_mean.weight"] * 30.0    # actions of order 0.3: the drones move
    return P.DevicePolicy(actor, critic, device=env.device, seed=seed)


@pytest.mark.parametrize("use_tp", [0, 1], ids=["plain", "predictor"])
def test_evaluate_equals_the_hand_loop(use_tp):
    N, L = 64, 6
    task = {"num_agents": 3, "env": {"num_envs": N, "max_episode_length": L}}
    env, hand = _make_env(task, use_tp), _make_env(task, use_tp)
    try:
        pol = _env_policy(env, 8)
        ev = evaluator.DeviceEvaluator(env, pol)
        info = ev.evaluate(seed=3)
        assert (ev.steps, ev.done_reads, ev.launches) == (L, 1, 1)                # the 24 statistics are one launch, one copy to the host
        # the hand loop: what a user writes from the reference's evaluate() (scripts/train.py:207-254)
        hand.set_seed(3)
        cur = hand.reset()
        stacked, dones = {k: [] for k in abi.STAT_NAMES}, []
        for _ in range(L):
            obs = cur[("agents", "observation")]
            out = pol.forward(obs["state_self"], obs.get("state_others", None), obs["cylinders"], deterministic=True)
            cur = hand.step(hand.rand_step_input(out.action))["next"]
            for k in abi.STAT_NAMES:
                stacked[k].append(hand.stats[k].clone())
            dones.append(cur["done"].clone())
        done = torch.stack(dones, dim=1)                                          # [N, L, 1]
        assert bool(done[:, -1].all()) and not bool(done[:, :-1].any())           # pure truncation
        first_done = torch.argmax(done.long(), dim=1)
        assert set(info) == {"eval/stats." + k for k in abi.STAT_NAMES} == {"eval/stats." + k for k in ev.stats}
        moved = 0
        for k in abi.STAT_NAMES:
            traj = torch.stack(stacked[k], dim=1)                                 # [N, L, 1]
            first = torch.take_along_dim(traj, first_done.reshape(first_done.shape + (1,) * (traj.ndim - 2)), dim=1).reshape(-1)
            assert ev.stats[k].shape == (N,) and LC.bits_equal(ev.stats[k], hand.stats[k].reshape(-1)), k
            assert LC.bits_equal(ev.stats[k], first), k
            EC.check_mean(info["eval/stats." + k], ev.stats[k].cpu().numpy(), None, k)
            moved += bool((traj[:, -1] != traj[:, 0]).any())
        assert moved >= 3                                                         # the statistics are not all constants of the episode
        again = ev.evaluate(seed=3)
        a, b = (np.array([d["eval/stats." + k] for k in abi.STAT_NAMES], np.float32) for d in (info, again))
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
        other = ev.evaluate(seed=4)
        assert any(other["eval/stats." + k] != info["eval/stats." + k] for k in abi.STAT_NAMES)   # ... and the seed is what seeds it
    finally:
        env.close()
        hand.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# training is undisturbed
def _training_side(with_eval):
    """Two collect -> train_rollout iterations (test_hip_collector.py's shapes, the learner on torch's global generators), optionally with an
    evaluation on a separate 32-env env between them: (info rows, every tensor a train_op changes)."""
    N, T, A = 64, 8, 3
    cfg = copy.deepcopy(LC.CFG)
    cfg.update(ppo_epochs=1, num_minibatches=16)
    env = _make_env({"num_agents": A, "env": {"num_envs": N}}, 1, seed=3)
    eval_env = _make_env({"num_agents": A, "env": {"num_envs": 32, "max_episode_length": 10}}, 1, seed=9)
    try:
        state = LC.clone_state(LC.make_state(A, 71), "cuda")
        pol = P.DevicePolicy(state["actor"], state["critic"], cfg, seed=4)
        L = learner.DeviceLearner(state["actor"], state["critic"], cfg, tp_net=env.TP, value_normalizer=state["vn"], generator=None,
                                  device_policy=pol)
        col = collector.DeviceCollector(env, pol, T)
        ev = evaluator.DeviceEvaluator(eval_env, pol, tp_net=env.TP)
        torch.manual_seed(77)                                    # both sides start the global generators (CPU and device) from one state
        infos = []
        for it in range(2):
            infos.append(L.train_rollout(**col.collect().learner_kwargs()))
            if with_eval and it == 0:
                res = ev.evaluate(seed=0)
                assert len(res) == abi.HNS_NUM_STATS and ev.steps == 10
                for k, v in eval_env.TP.state_dict().items():                    # the evaluation env took the trained predictor
                    assert LC.bits_equal(v, env.TP.state_dict()[k]), k
        tensors = {k: v.detach().clone() for k, v in LC.state_tensors(dict(state, tp=env.TP), LC.learner_opts(L)).items()}
        return infos, tensors
    finally:
        env.close()
        eval_env.close()


def test_an_evaluation_between_two_iterations_leaves_training_bit_for_bit():
    plain, plain_t = _training_side(False)
    mixed, mixed_t = _training_side(True)
    for it, (a, b) in enumerate(zip(plain, mixed)):
        assert set(a) == set(b) == {f"drone/{k}" for k in learner.INFO_KEYS}
        x, y = (np.array([i[k] for k in sorted(i)], np.float64) for i in (a, b))
        assert np.array_equal(x, y, equal_nan=True), (it, a, b)
    LC.assert_same_state(mixed_t, plain_t, "with an evaluation between the iterations")


def test_an_evaluation_on_the_training_env_puts_it_back_and_restarts_the_collector():
    N, T, L = 64, 8, 6
    env = _make_env({"num_agents": 3, "env": {"num_envs": N, "max_episode_length": L}}, 1, seed=3)
    try:
        pol = _env_policy(env, 8)
        col = collector.DeviceCollector(env, pol, T)
        col.collect()
        env.eval()                                               # (whatever the flag is, it comes back)
        before = (env.training, env.seed, env.reset_epoch)
        assert before[0] is False and before[1] == 3
        cpu_rng, dev_rng = torch.get_rng_state().clone(), torch.cuda.get_rng_state(env.device).clone()
        calls = []
        reset = env.reset
        env.reset = lambda td=None, **kw: (calls.append(td is None), reset(td, **kw))[1]
        evaluator.DeviceEvaluator(env, pol, collector=col).evaluate(seed=5)
        assert (env.training, env.seed, env.reset_epoch) == before
        assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(env.device), dev_rng)
        assert calls == [True]
        env.train()
        col.collect()
        assert calls[1] is True                                  # the collector's next collect() starts from a full reset
        assert env.reset_epoch > before[2]
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the example script
def test_the_training_example_evaluates_checkpoints_and_resumes(tmp_path):
    script = os.path.join(ROOT, "examples", "train_device.py")
    base = [sys.executable, script, "--envs", "64", "--train-every", "8", "--eval-interval", "1", "--eval-envs", "32", "--save-interval", "1"]
    first = subprocess.run(base + ["--iterations", "2", "--checkpoint-dir", str(tmp_path)], capture_output=True, text=True, timeout=240)
    assert first.returncode == 0, first.stdout + first.stderr
    assert first.stdout.count("eval/stats.success") == 3         # i = 0, i = 1 and once after the loop
    assert sorted(os.listdir(tmp_path)) == ["checkpoint_1024.pt", "checkpoint_512.pt", "checkpoint_final.pt"]
    again = tmp_path / "again"
    second = subprocess.run(base + ["--iterations", "1", "--checkpoint-dir", str(again), "--resume", str(tmp_path / "checkpoint_final.pt")],
                            capture_output=True, text=True, timeout=240)
    assert second.returncode == 0, second.stdout + second.stderr
    assert second.stdout.count("eval/stats.success") == 2 and os.path.exists(again / "checkpoint_final.pt")
