"""CentralCriticDeviceLearner, the collector's state segment and the evaluator on an MI355X, at 8 envs x 4 steps x 3 agents, 2 minibatches x 2
epochs, the predictor off and on (a two-step prediction horizon, so that four steps hold windows): train_op against the hand-driven loop bit
for bit (tests/central_learner_cases.py), the stored state against a hand-driven env loop, the other policies' storage untouched.
DESIGN.md §7.20."""
import copy

import pytest
import torch

import central_learner_cases as CC
import learner_cases as LC
from hns_amd import abi, collector, config
from hns_amd import policy as P

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
