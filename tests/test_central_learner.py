"""CentralCriticDeviceLearner and the collector's state segment on the CPU: train_op against the hand-driven loop bit for bit
(tests/central_learner_cases.py), the tensordict entry, the checkpoint under the reference's names, the refusals.  DESIGN.md §7.20."""
import numpy as np
import pytest
import torch

import central_learner_cases as CC
import learner_cases as LC
from hns_amd import collector, learner
from hns_amd import policy as P

N, T, A, D, K = 8, 4, 3, 35, 5


@pytest.fixture(scope="module")
def case():
    state = CC.make_state(A, D, 31)
    return state, CC.make_rollout(state, N, T, A, D, K, 32)


def test_train_rollout_equals_the_hand_loop(case):
    CC.check_train_op_equals_the_hand_loop(*case)


def test_train_op_reads_the_state_groups_of_the_tensordict(case):
    state, ro = case
    a, b = CC.clone_state(state), CC.clone_state(state)
    La, Lb = CC.make_learner(a, seed=5), CC.make_learner(b, seed=5)
    ia, ib = La.train_op(CC.as_tensordict(ro)), Lb.train_rollout(**ro)
    assert ia == ib and set(ia) == {f"drone/{k}" for k in learner.INFO_KEYS if k != "TP_loss"}
    LC.assert_same_state(CC.state_tensors(a, CC.learner_opts(La)), CC.state_tensors(b, CC.learner_opts(Lb)), "train_op against train_rollout")


def test_checkpoint_is_the_references_with_the_central_critics_names(case):
    state, ro = case
    a = CC.clone_state(state)
    L = CC.make_learner(a, seed=5)
    L.train_rollout(**ro)
    sd = L.state_dict()
    assert set(sd) == {"critic", "actor_params", "value_normalizer", "actor_opt", "critic_opt"}
    assert set(sd["critic"]) == set(P.CENTRAL_CRITIC_NAMES) and sd["critic"]["v_out.weight"].shape == (A, 128)
    assert len(sd["critic_opt"]["param_groups"][0]["params"]) == 20
    b = CC.clone_state(state)
    L2 = CC.make_learner(b, seed=5)
    L2.load_state_dict({k: (v if "opt" in k else {n: t.clone() for n, t in v.items()}) for k, v in sd.items()})
    for k in a["critic"]:
        assert torch.equal(a["critic"][k], b["critic"][k]), k
    pol = P.CentralCriticDevicePolicy.from_checkpoint(sd, cfg=CC.CFG)
    assert pol.num_agents == A
    i1, i2 = L.train_rollout(**ro), L2.train_rollout(**ro)      # (the generators are at different states: the loaded learner's is fresh)
    assert set(i1) == set(i2)


def test_refusals():
    state = CC.make_state(A, D, 31)
    E = P.PolicyConfigError
    mk = lambda cfg=CC.CFG, **kw: learner.CentralCriticDeviceLearner(state["actor"], state["critic"], cfg, value_normalizer=state["vn"], **kw)   # noqa: E731
    with pytest.raises(NotImplementedError, match="group"):
        mk(group="world")
    with pytest.raises(E, match="critic_input"):
        mk({**CC.CFG, "critic_input": "obs"})
    with pytest.raises(E, match="share_actor"):
        mk({**CC.CFG, "share_actor": False})
    with pytest.raises(E, match="rnn"):
        mk({**CC.CFG, "critic": {**CC.CFG["critic"], "rnn": {"cls": "gru"}}})
    with pytest.raises(E, match="num_critics"):
        mk({**CC.CFG, "critic": {**CC.CFG["critic"], "num_critics": 2}})
    obs_actor, obs_critic = P.random_parameters(D, A, 1)
    with pytest.raises(E, match="CentralCriticDevicePolicy"):
        mk(device_policy=P.DevicePolicy(obs_actor, obs_critic))
    with pytest.raises(E, match="shared non-recurrent"):
        mk(device_policy=P.PerAgentDevicePolicy(P.random_parameters_per_agent(D, A, 1)[0], obs_critic))
    with pytest.raises(E):
        learner.CentralCriticDeviceLearner(state["actor"], obs_critic, CC.CFG)                        # the obs critic's tensors
    pol = P.CentralCriticDevicePolicy(state["actor"], state["critic"])
    # DeviceLearner keeps refusing the configuration and the policy
    with pytest.raises(E, match="centralised critic"):
        learner.DeviceLearner(state["actor"], state["critic"], CC.CFG)
    with pytest.raises(E, match="CentralCriticDeviceLearner"):
        learner.DeviceLearner(obs_actor, obs_critic, LC.CFG, device_policy=pol)
    L = mk(device_policy=pol)
    ro = CC.make_rollout(state, N, T, A, D, K, 32)
    with pytest.raises(ValueError, match="state_drones"):
        L.train_rollout(**{k: v for k, v in ro.items() if k not in ("state_drones", "next_state_last")})
    with pytest.raises(ValueError, match="state_drones"):
        L.train_rollout(**{**ro, "state_drones": ro["state_drones"][:, :2]})


class _Env:
    """The collector's env surface on the CPU: observations and state are functions of a step counter; an episode is `L` steps."""
    max_episode_length = 6

    def __init__(self):
        self.batch_size, self.t = [N], 0

    def _td(self):
        from hns_amd.tensordict_shim import TensorDict
        g = torch.Generator().manual_seed(100 + self.t)
        r = lambda *s: torch.randn(*s, generator=g)              # noqa: E731
        obs = {"state_self": r(N, A, 1, D), "state_others": r(N, A, A - 1, 3), "cylinders": r(N, A, K, 5)}
        done = torch.full((N, 1), self.t > 0 and self.t % self.max_episode_length == 0)
        return TensorDict({"agents": {"observation": obs, "state": {"state_drones": r(N, A, D), "cylinders": obs["cylinders"]},
                                      "reward": r(N, A, 1)}, "done": done}, self.batch_size)

    def reset(self, td=None):
        return self._td()

    def step(self, td):
        from hns_amd.tensordict_shim import TensorDict
        self.t += 1
        return TensorDict({"next": self._td()}, self.batch_size)


def test_collector_stores_the_state_the_policy_read():
    state = CC.make_state(A, D, 31)
    pol = P.CentralCriticDevicePolicy(state["actor"], state["critic"], seed=3)
    col = collector.DeviceCollector(_Env(), pol, T)
    st = col.collect()
    kw = st.learner_kwargs()
    assert kw["state_drones"].shape == (N, T, A, D) and kw["next_state_last"].shape == (N, A, D)
    hand, ref = _Env(), P.CentralCriticDevicePolicy(state["actor"], state["critic"], seed=3)
    cur = hand.reset()
    for t in range(T):
        obs, sd = cur[("agents", "observation")], cur[("agents", "state")]["state_drones"]
        out = ref.forward(obs["state_self"], obs["state_others"], obs["cylinders"], sd)
        assert torch.equal(kw["state_drones"][:, t], sd) and torch.equal(kw["state_value"][:, t], out.value), t
        assert torch.equal(kw["action"][:, t], out.action), t
        cur = hand.step(None)["next"]
    assert torch.equal(kw["next_state_last"], cur[("agents", "state")]["state_drones"])
    info = learner.CentralCriticDeviceLearner(state["actor"], state["critic"], CC.CFG, value_normalizer=state["vn"], device_policy=pol).train_rollout(**kw)
    assert np.isfinite(list(info.values())).all()
    # every other policy: the parent's storage keys, no state
    actor, critic = P.random_parameters(D, A, 1)
    plain = collector.DeviceCollector(_Env(), P.DevicePolicy(actor, critic, seed=3), T).collect()
    assert set(plain.data) == {"obs_self", "obs_others", "obs_cylinders", "action", "log_probs", "state_value", "reward", "done"}
    assert set(plain.last) == {"obs_self", "obs_others", "obs_cylinders"} and "state_drones" not in plain.learner_kwargs()
    with pytest.raises(ValueError, match="recurrent"):
        collector.DeviceCollector(_Env(), type("R", (), {"recurrent": True, "needs_state": True})(), 16)
