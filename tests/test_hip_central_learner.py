"""CentralCriticDeviceLearner, the collector's state segment and the evaluator on an MI355X, at 8 envs x 4 steps x 3 agents, 2 minibatches x 2
epochs, the predictor off and on (a two-step prediction horizon, so that four steps hold windows): train_op against the hand-driven loop bit
for bit (tests/central_learner_cases.py), the stored state against a hand-driven env loop, the other policies' storage untouched; the state
segment across episode boundaries (episodes of 6 steps, three rollouts of 4: a boundary in mid-rollout and one on a rollout's last step).
DESIGN.md §7.20."""
import copy

import pytest
import torch

import central_learner_cases as CC
import learner_cases as LC
from hns_amd import abi, collector, config
from hns_amd import policy as P
from hns_amd.tensordict_shim import TensorDict

pytestmark = pytest.mark.gpu

N, T, A = 8, 4, 3


def _env(use_tp, seed=3, critic_input="state"):
    from hns_amd.env import HideAndSeek
    torch.manual_seed(seed + 100)                                # the predictor's initial weights come from the global generator
    cfg = config.make_cfg({"num_agents": A, "future_predcition_step": 2, "env": {"num_envs": N, "max_episode_length": 6}},
                          algo={"use_TP_net": int(use_tp), "critic_input": critic_input})
    env = HideAndSeek(cfg, headless=True)
    env.set_seed(seed)
    return env


def _dim(env):
    return abi.self_dim(env.num_targets) + (3 * env.tp_future_step * env.num_targets if env.use_TP_net else 0)


def _policy(state, seed=4):
    return P.CentralCriticDevicePolicy(state["actor"], state["critic"], CC.CFG, seed=seed)


@pytest.mark.parametrize("use_tp", [0, 1], ids=["plain", "predictor"])
def test_collector_and_train_op_against_the_hand_loops(use_tp):
    env, hand = _env(use_tp), _env(use_tp)
    try:
        D = _dim(env)
        state = CC.make_state(A, D, 71, "cuda", tp=env.TP if use_tp else None)
        pol = _policy(state)
        col = collector.DeviceCollector(env, pol, T)
        st = col.collect()
        assert st.launches == 2 * T + 1                          # the state is one more segment of the pre-step store, not one more launch
        kw = st.learner_kwargs()
        assert kw["state_drones"].shape == (N, T, A, D) and kw["next_state_last"].shape == (N, A, D)
        # the hand-driven loop on a second env from the same seed, the same policy call by call
        ref = _policy(state)
        cur = hand.reset()
        for t in range(T):
            obs, sd = cur[("agents", "observation")], cur[("agents", "state")]["state_drones"]
            assert LC.bits_equal(kw["state_drones"][:, t], sd) and LC.bits_equal(kw["obs_self"][:, t], obs["state_self"]), t
            out = ref.forward(obs["state_self"], obs["state_others"], obs["cylinders"], sd)
            for name, x in (("action", out.action), ("log_probs", out.log_prob), ("state_value", out.value)):
                assert LC.bits_equal(kw[name][:, t], x), (t, name)
            cur = hand.step(hand.rand_step_input(out.action))["next"]
        assert LC.bits_equal(kw["next_state_last"], cur[("agents", "state")]["state_drones"])
        assert float(kw["state_drones"].abs().max()) > 0 and not LC.bits_equal(kw["state_drones"][:, 0], kw["state_drones"][:, -1])
        # train_op on that storage: the learner against the calls driven by hand, twice
        ro = {k: (v.clone() if torch.is_tensor(v) else tuple(x.clone() if x is not None else None for x in v)) for k, v in kw.items()}
        ro["agent_done"] = None
        L, after = CC.check_train_op_equals_the_hand_loop(state, ro)
        assert L.policy.central and (L.tp_opt is not None) == bool(use_tp)
    finally:
        env.close()
        hand.close()


def test_the_state_segment_across_episode_boundaries():
    """max_episode_length 6, T = 4, three collects: steps 1-4, 5-8 (the boundary after step 6, slot 1: slot 2 holds the POST-reset state, bit
    for bit the hand loop's, `done` is from before the reset) and 9-12 (the boundary on the last step: next_state_last is the PRE-reset state,
    as next_obs_last is the pre-reset observation, and the carried state is the reset's)."""
    env, hand = _env(0), _env(0)
    try:
        D = _dim(env)
        state = CC.make_state(A, D, 71, "cuda")
        col = collector.DeviceCollector(env, _policy(state), T)
        ref, cur = _policy(state), hand.reset()
        for call in range(3):
            st = col.collect()
            kw = st.learner_kwargs()
            assert st.launches == (call + 1) * (2 * T + 1)       # still one pre-step store, one post-step store a step, one last store
            for t in range(T):
                obs, sd = cur[("agents", "observation")], cur[("agents", "state")]["state_drones"]
                assert LC.bits_equal(kw["state_drones"][:, t], sd) and LC.bits_equal(kw["obs_self"][:, t], obs["state_self"]), (call, t)
                out = ref.forward(obs["state_self"], obs["state_others"], obs["cylinders"], sd)
                for name, x in (("action", out.action), ("log_probs", out.log_prob), ("state_value", out.value)):
                    assert LC.bits_equal(kw[name][:, t], x), (call, t, name)
                nxt = hand.step(hand.rand_step_input(out.action))["next"]
                done = nxt["done"].clone()
                step = call * T + t + 1
                assert bool(done.all()) == (step % 6 == 0) and bool(done.any()) == (step % 6 == 0), (call, t)
                assert torch.equal(kw["done"][:, t], done), (call, t)                                   # done as it was before the reset
                if t == T - 1:
                    last_state = nxt[("agents", "state")]["state_drones"].clone()
                    last_self = nxt[("agents", "observation")]["state_self"].clone()
                pre = nxt[("agents", "state")]["state_drones"].clone()
                cur = hand.reset(TensorDict({"_reset": done.reshape(-1, 1)}, hand.batch_size)) if bool(done.any()) else nxt
                if bool(done.any()):
                    assert not LC.bits_equal(cur[("agents", "state")]["state_drones"], pre), (call, t)  # the reset moved the drones
            assert LC.bits_equal(kw["next_state_last"], last_state) and LC.bits_equal(kw["next_obs_last"][0], last_self), call
            assert bool(kw["done"].any()) == (call > 0)
            if call == 1:
                assert bool(kw["done"][:, 1].all()) and not bool(kw["done"][:, [0, 2, 3]].any())
            if call == 2:
                # the rollout ended on the boundary: the carried state is the reset's, next_state_last the step's own next state
                assert bool(kw["done"][:, 3].all()) and not bool(kw["done"][:, :3].any())
                assert not LC.bits_equal(kw["next_state_last"], cur[("agents", "state")]["state_drones"])
                assert LC.bits_equal(col._cur[("agents", "state")]["state_drones"], cur[("agents", "state")]["state_drones"])
    finally:
        env.close()
        hand.close()


def test_other_policies_keep_their_storage():
    """With a DevicePolicy the collector stores what it stored before the state segment existed: the same names, the same launches, the
    bits of a hand-driven loop — on an env that writes the state, too."""
    env, hand = _env(0), _env(0)
    try:
        D = _dim(env)
        actor, critic = P.random_parameters(D, A, 5)
        mk = lambda: P.DevicePolicy(copy.deepcopy(actor), copy.deepcopy(critic), device=env.device, seed=4)      # noqa: E731
        st = collector.DeviceCollector(env, mk(), T).collect()
        assert set(st.data) == {"obs_self", "obs_others", "obs_cylinders", "action", "log_probs", "state_value", "reward", "done"}
        assert set(st.last) == {"obs_self", "obs_others", "obs_cylinders"} and st.launches == 2 * T + 1
        assert set(st.learner_kwargs()) == {"obs_self", "obs_others", "obs_cylinders", "action", "log_probs", "state_value", "next_obs_last",
                                            "reward", "done"}
        ref, cur = mk(), hand.reset()
        for t in range(T):
            obs = cur[("agents", "observation")]
            out = ref.forward(obs["state_self"], obs["state_others"], obs["cylinders"])
            for name, x in (("obs_cylinders", obs["cylinders"]), ("action", out.action), ("log_probs", out.log_prob), ("state_value", out.value)):
                assert LC.bits_equal(st.data[name][:, t], x), (t, name)
            nxt = hand.step(hand.rand_step_input(out.action))["next"]
            assert LC.bits_equal(st.data["reward"][:, t], nxt[("agents", "reward")]), t
            cur = nxt
    finally:
        env.close()
        hand.close()
