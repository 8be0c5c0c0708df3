"""PerAgentCentralCriticDeviceLearner and the collector over PerAgentCentralCriticDevicePolicy on an MI355X, at 8 envs x 4 steps x 3 agents,
2 minibatches x 2 epochs, the predictor off and on (a two-step prediction horizon, so that four steps hold windows): the collector's storage
against a hand-driven env loop, train_rollout against the hand-driven calls bit for bit (tests/per_agent_central_cases.py), a cached workspace
past one row range and then at one tile, the critic's tensors against CentralCriticDeviceLearner's, and one collect across an episode
boundary.  DESIGN.md §7.21."""
import copy

import numpy as np
import pytest
import torch

import central_cases as CE
import central_learner_cases as CC
import learner_cases as LC
import per_agent_cases as PA
import per_agent_central_cases as PC
from hns_amd import abi, collector, config
from hns_amd import policy as P
from hns_amd.tensordict_shim import TensorDict

pytestmark = pytest.mark.gpu

N, T, A = 8, 4, 3


def _env(use_tp, seed=3):
    from hns_amd.env import HideAndSeek
    torch.manual_seed(seed + 100)                                # the predictor's initial weights come from the global generator
    cfg = config.make_cfg({"num_agents": A, "future_predcition_step": 2, "env": {"num_envs": N, "max_episode_length": 6}},
                          algo={"use_TP_net": int(use_tp), "critic_input": "state", "share_actor": False})
    env = HideAndSeek(cfg, headless=True)
    env.set_seed(seed)
    return env


def _dim(env):
    return abi.self_dim(env.num_targets) + (3 * env.tp_future_step * env.num_targets if env.use_TP_net else 0)


@pytest.mark.parametrize("use_tp", [0, 1], ids=["plain", "predictor"])
def test_collector_and_train_op_against_the_hand_loops(use_tp):
    env, hand = _env(use_tp), _env(use_tp)
    try:
        D = _dim(env)
        state = PC.make_state(A, D, 71, "cuda", tp=env.TP if use_tp else None)
        pol = PC.make_policy(state, seed=4)
        st = collector.DeviceCollector(env, pol, T).collect()
        assert st.launches == 2 * T + 1                          # the store plan is the centralised critic's, unchanged
        kw = st.learner_kwargs()
        assert kw["state_drones"].shape == (N, T, A, D) and kw["next_state_last"].shape == (N, A, D)
        ref = PC.make_policy(state, seed=4)
        cur = hand.reset()
        for t in range(T):
            obs, sd = cur[("agents", "observation")], cur[("agents", "state")]["state_drones"]
            assert LC.bits_equal(kw["state_drones"][:, t], sd) and LC.bits_equal(kw["obs_self"][:, t], obs["state_self"]), t
            out = ref.forward(obs["state_self"], obs["state_others"], obs["cylinders"], sd)
            for name, x in (("action", out.action), ("log_probs", out.log_prob), ("state_value", out.value)):
                assert LC.bits_equal(kw[name][:, t], x), (t, name)
            cur = hand.step(hand.rand_step_input(out.action))["next"]
        assert LC.bits_equal(kw["next_state_last"], cur[("agents", "state")]["state_drones"])
        # train_rollout on that storage: the learner against the calls driven by hand, twice
        ro = {k: (v.clone() if torch.is_tensor(v) else tuple(x.clone() if x is not None else None for x in v)) for k, v in kw.items()}
        ro["agent_done"] = None
        L, after = PC.check_train_op_equals_the_hand_loop(state, ro)
        assert L.policy.central and L.policy.per_agent and (L.tp_opt is not None) == bool(use_tp)
        # train_op: the tensordict entry reads the same tensors
        if not use_tp:
            a, b = PC.clone_state(state), PC.clone_state(state)
            La, Lb = PC.make_learner(a, seed=5), PC.make_learner(b, seed=5)
            assert La.train_op(CC.as_tensordict(ro)) == Lb.train_rollout(**ro)
            LC.assert_same_state(PC.state_tensors(a, PC.learner_opts(La)), PC.state_tensors(b, PC.learner_opts(Lb)), "train_op against train_rollout")
    finally:
        env.close()
        hand.close()


def test_train_rollout_through_the_cached_workspaces_is_the_hand_driven_sequence_bit_for_bit():
    """53 envs x 29 steps = 1 537 env-steps in ONE minibatch — the critic at tps 2 with a last row range of one tile with one live row, the
    actor at 49 tiles per agent in row ranges of 4 — one epoch, predictor off; then 8 x 4 = 32 env-steps (one tile per agent, one critic
    tile) in the two workspaces the first call cached."""
    D, K = 20, 5
    cfg = {**PC.CFG, "num_minibatches": 1, "ppo_epochs": 1}
    assert CE.central_plan(53 * 29)[:3] == (49, 2, 25) and CE.central_plan(8 * 4)[:3] == (1, 1, 1)
    assert PA.agents_plan(53 * 29, A)[:3] == (49, 4, 13) and PA.agents_plan(8 * 4, A)[:3] == (1, 1, 1)
    state = PC.make_state(A, D, 81, "cuda")
    a, b = PC.clone_state(state), PC.clone_state(state)
    L = PC.make_learner(a, cfg, seed=5)
    opts, gen = PC.hand_optimisers(b), torch.Generator(device="cuda").manual_seed(5)
    sizes = None
    for (n, t), seed in (((53, 29), 82), ((8, 4), 83)):
        ro = LC.to_device(PC.make_rollout(state, n, t, A, D, K, seed), "cuda")
        got = L.train_rollout(**ro)
        want = PC.hand_train_op(b, opts, ro, gen, cfg)
        torch.cuda.synchronize()
        for k, v in want.items():
            assert np.float32(got[f"drone/{k}"]) == np.float32(v), ((n, t), k, got[f"drone/{k}"], v)
        LC.assert_same_state(PC.state_tensors(a, PC.learner_opts(L)), PC.state_tensors(b, opts), f"train_rollout of {n} x {t} against the hand sequence")
        if sizes is None:
            sizes = L._ws["actor"].numel(), L._ws["critic"].numel()
            assert sizes == (PA.agents_workspace_bytes(1537, D, A, K), CE.central_workspace_bytes(1537, D, A, K))
    assert (L._ws["actor"].numel(), L._ws["critic"].numel()) == sizes                               # the second rollout ran in the first's workspaces
    assert sizes[0] > PA.agents_workspace_bytes(32, D, A, K) and sizes[1] > CE.central_workspace_bytes(32, D, A, K)
    for net, least in (("actor", 20), ("critic", 18)):
        assert sum(not torch.equal(a[net][k], state[net][k]) for k in a[net]) >= least, net


def test_the_critic_block_never_reads_the_actor():
    """The critic's tensors and its Adam state after one rollout equal CentralCriticDeviceLearner's for the same rollout tensors, generator
    seed and critic (beside another, shared, actor)."""
    D, K = 35, 5
    state = PC.make_state(A, D, 31, "cuda")
    ro = LC.to_device(PC.make_rollout(state, N, T, A, D, K, 32), "cuda")
    a = PC.clone_state(state)
    La = PC.make_learner(a, seed=5)
    La.train_rollout(**ro)
    shared = CC.make_state(A, D, 77, "cuda")
    b = {"actor": shared["actor"], "critic": PC.clone_state(state)["critic"], "tp": None, "vn": copy.deepcopy(state["vn"])}
    Lb = CC.make_learner(b, seed=5)
    Lb.train_rollout(**ro)
    torch.cuda.synchronize()
    for k in a["critic"]:
        assert LC.bits_equal(a["critic"][k], b["critic"][k]), k
        for s, v in La.critic_opt.state[a["critic"][k]].items():
            assert LC.bits_equal(v, Lb.critic_opt.state[b["critic"][k]][s]), (k, s)
    assert sum(not torch.equal(a["critic"][k], state["critic"][k]) for k in a["critic"]) >= 18


def test_one_collect_across_an_episode_boundary():
    """max_episode_length 6, ONE collect of 8 steps: the boundary after step 6 — slot 6 holds the POST-reset observation and state, bit for
    bit the hand loop's, `done` is from before the reset — and every stored tensor equals the hand-driven loop; next_state_last is the last
    step's own next state."""
    steps = 8
    env, hand = _env(0), _env(0)
    try:
        D = _dim(env)
        state = PC.make_state(A, D, 71, "cuda")
        st = collector.DeviceCollector(env, PC.make_policy(state, seed=4), steps).collect()
        kw = st.learner_kwargs()
        assert st.launches == 2 * steps + 1
        ref, cur = PC.make_policy(state, seed=4), hand.reset()
        for t in range(steps):
            obs, sd = cur[("agents", "observation")], cur[("agents", "state")]["state_drones"]
            for name, x in (("state_drones", sd), ("obs_self", obs["state_self"]), ("obs_others", obs["state_others"]), ("obs_cylinders", obs["cylinders"])):
                assert LC.bits_equal(kw[name][:, t], x), (t, name)
            out = ref.forward(obs["state_self"], obs["state_others"], obs["cylinders"], sd)
            for name, x in (("action", out.action), ("log_probs", out.log_prob), ("state_value", out.value)):
                assert LC.bits_equal(kw[name][:, t], x), (t, name)
            nxt = hand.step(hand.rand_step_input(out.action))["next"]
            done = nxt["done"].clone()
            assert bool(done.all()) == bool(done.any()) == (t + 1 == 6), t
            assert torch.equal(kw["done"][:, t], done) and LC.bits_equal(kw["reward"][:, t], nxt[("agents", "reward")]), t
            if t == steps - 1:
                last = nxt
            pre = nxt[("agents", "state")]["state_drones"].clone()
            cur = hand.reset(TensorDict({"_reset": done.reshape(-1, 1)}, hand.batch_size)) if bool(done.any()) else nxt
            if bool(done.any()):
                assert not LC.bits_equal(cur[("agents", "state")]["state_drones"], pre), t                 # the reset moved the drones
        assert LC.bits_equal(kw["next_state_last"], last[("agents", "state")]["state_drones"])
        lo = last[("agents", "observation")]
        for got, want in zip(kw["next_obs_last"], (lo["state_self"], lo["state_others"], lo["cylinders"])):
            assert LC.bits_equal(got, want)
        assert bool(kw["done"][:, 5].all()) and not bool(kw["done"][:, [0, 1, 2, 3, 4, 6, 7]].any())
    finally:
        env.close()
        hand.close()
