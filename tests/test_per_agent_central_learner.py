"""PerAgentCentralCriticDeviceLearner on the CPU, at central_learner_cases.py's smallest case (8 envs x 4 steps x 3 agents, 2 minibatches x 2
epochs) extended to stacked actors: train_rollout against the hand-driven calls bit for bit (tests/per_agent_central_cases.py) with the
predictor off and on, train_op's tensordict entry, state_dict and the checkpoint round trips, the collector over the new policy, the refusals.
DESIGN.md §7.21."""
import copy

import numpy as np
import pytest
import torch

import central_learner_cases as CC
import learner_cases as LC
import per_agent_central_cases as PC
from hns_amd import collector, learner
from hns_amd import policy as P

N, T, A, D, K = 8, 4, 3, 35, 5


@pytest.fixture(scope="module")
def cases():
    out = {}
    for use_tp in (False, True):
        state = PC.make_state(A, D, 31, tp=PC.make_tp(A, 33) if use_tp else None)
        out[use_tp] = (state, PC.make_rollout(state, N, T, A, D, K, 32, tp=use_tp))
    return out


@pytest.mark.parametrize("use_tp", [False, True], ids=["plain", "predictor"])
def test_train_rollout_equals_the_hand_loop(cases, use_tp):
    """Parameters, Adam state, ValueNorm1's buffers (and the predictor's tensors and optimiser) and the info row against
    update_actor_per_agent + update_critic_central driven by hand."""
    L, _ = PC.check_train_op_equals_the_hand_loop(*cases[use_tp])
    assert type(L.policy) is P.PerAgentCentralCriticDevicePolicy and (L.tp_opt is not None) == use_tp
    assert len(L.actor_opt.param_groups[0]["params"]) == 23 and len(L.critic_opt.param_groups[0]["params"]) == 20
    actor_t, critic_t = L._network_tensors()
    assert len(actor_t) == 23 and all(t.shape[0] == A for t in actor_t) and len(critic_t) == 20


def test_the_critic_block_never_reads_the_actor(cases):
    """The critic's tensors after one rollout are CentralCriticDeviceLearner's for the same rollout tensors, generator seed and critic."""
    state, ro = cases[False]
    a = PC.clone_state(state)
    PC.make_learner(a, seed=5).train_rollout(**ro)
    shared = CC.make_state(A, D, 77)
    b = {"actor": shared["actor"], "critic": PC.clone_state(state)["critic"], "tp": None, "vn": copy.deepcopy(state["vn"])}
    CC.make_learner(b, seed=5).train_rollout(**ro)
    for k in a["critic"]:
        assert LC.bits_equal(a["critic"][k], b["critic"][k]), k
    assert any(not torch.equal(a["critic"][k], state["critic"][k]) for k in a["critic"])


def test_train_op_reads_the_state_groups_of_the_tensordict(cases):
    state, ro = cases[False]
    a, b = PC.clone_state(state), PC.clone_state(state)
    La, Lb = PC.make_learner(a, seed=5), PC.make_learner(b, seed=5)
    ia, ib = La.train_op(CC.as_tensordict(ro)), Lb.train_rollout(**ro)
    assert ia == ib and set(ia) == {f"drone/{k}" for k in learner.INFO_KEYS if k != "TP_loss"}
    LC.assert_same_state(PC.state_tensors(a, PC.learner_opts(La)), PC.state_tensors(b, PC.learner_opts(Lb)), "train_op against train_rollout")


def test_state_dict_and_checkpoint_round_trip(cases, tmp_path):
    """state_dict -> load_state_dict into a fresh learner, and the checkpoint -> from_checkpoint: bit for bit, under the reference's names
    (stacked actor_params beside the central critic's)."""
    state, ro = cases[False]
    a = PC.clone_state(state)
    L = PC.make_learner(a, seed=5)
    L.train_rollout(**ro)
    sd = L.state_dict()
    assert set(sd) == {"critic", "actor_params", "value_normalizer", "actor_opt", "critic_opt"}
    assert set(sd["critic"]) == set(P.CENTRAL_CRITIC_NAMES) and sd["critic"]["v_out.weight"].shape == (A, 128)
    assert set(sd["actor_params"]) == set(P.ACTOR_NAMES) and all(v.shape[0] == A for v in sd["actor_params"].values())
    assert len(sd["actor_opt"]["param_groups"][0]["params"]) == 23 and len(sd["critic_opt"]["param_groups"][0]["params"]) == 20
    path = tmp_path / "learner.pt"
    torch.save(sd, path)
    loaded = torch.load(path, map_location="cpu", weights_only=False)
    b = PC.clone_state(PC.make_state(A, D, 99))
    L2 = PC.make_learner(b, seed=5)
    L2.load_state_dict(loaded)
    LC.assert_same_state(PC.state_tensors(b, PC.learner_opts(L2)), PC.state_tensors(a, PC.learner_opts(L)), "state_dict round trip")
    pol = P.PerAgentCentralCriticDevicePolicy.from_checkpoint(str(path), cfg=PC.CFG)
    assert pol.num_agents == A
    assert all(torch.equal(pol.actor_p[P.ACTOR_NAMES[k]], v) for k, v in a["actor"].items())
    assert all(torch.equal(pol.critic_p[P.CENTRAL_CRITIC_NAMES[k]], v) for k, v in a["critic"].items())
    # both learners go on from the same state: with generators at the same state, the same bits
    L.generator.manual_seed(9), L2.generator.manual_seed(9)
    assert L.train_rollout(**ro) == L2.train_rollout(**ro)
    LC.assert_same_state(PC.state_tensors(b, PC.learner_opts(L2)), PC.state_tensors(a, PC.learner_opts(L)), "the rollout after the round trip")


def test_refusals(cases):
    state, ro = cases[False]
    E = P.PolicyConfigError
    new = learner.PerAgentCentralCriticDeviceLearner
    mk = lambda cfg=PC.CFG, **kw: new(state["actor"], state["critic"], cfg, value_normalizer=state["vn"], **kw)       # noqa: E731
    with pytest.raises(NotImplementedError, match="no data-parallel form"):
        mk(group="world")
    with pytest.raises(E, match="critic_input"):
        mk({**PC.CFG, "critic_input": "obs"})
    with pytest.raises(E, match="share_actor"):
        mk({**PC.CFG, "share_actor": True})
    with pytest.raises(E, match="rnn"):
        mk({**PC.CFG, "critic": {**PC.CFG["critic"], "rnn": {"cls": "gru"}}})
    with pytest.raises(E, match="rnn"):
        mk({**PC.CFG, "actor": {**PC.CFG["actor"], "rnn": {"cls": "gru"}}})
    with pytest.raises(E, match="num_critics"):
        mk({**PC.CFG, "critic": {**PC.CFG["critic"], "num_critics": 2}})
    with pytest.raises(E, match="lr_scheduler"):
        mk({**PC.CFG, "actor": {**PC.CFG["actor"], "lr_scheduler": "x"}})
    with pytest.raises(NotImplementedError, match="weight_decay"):
        mk({**PC.CFG, "critic": {**PC.CFG["critic"], "weight_decay": 0.1}})
    shared_actor, obs_critic = P.random_parameters(D, A, 1)
    stacked = P.random_parameters_per_agent(D, A, 1)[0]
    central = P.random_parameters_central(D, A, 1)[1]
    for pol in (P.DevicePolicy(shared_actor, obs_critic), P.PerAgentDevicePolicy(stacked, obs_critic), P.CentralCriticDevicePolicy(shared_actor, central)):
        with pytest.raises(E, match="PerAgentCentralCriticDevicePolicy"):
            mk(device_policy=pol)
    with pytest.raises(E, match="non-recurrent"):
        mk(device_policy=type("R", (), {"recurrent": True, "per_agent": True, "central": True})())
    with pytest.raises(E):
        new(shared_actor, state["critic"], PC.CFG)                               # a shared actor's tensors
    with pytest.raises(E):
        new(state["actor"], obs_critic, PC.CFG)                                  # the obs critic's tensors
    ok = PC.make_policy(state)
    # the two parents and DeviceLearner keep refusing the policy and the configuration
    with pytest.raises(E, match="shared non-recurrent"):
        learner.CentralCriticDeviceLearner(shared_actor, central, CC.CFG, device_policy=ok)
    with pytest.raises(E, match="share_actor"):
        learner.CentralCriticDeviceLearner(shared_actor, central, PC.CFG)
    with pytest.raises(E, match="centralised critic"):
        learner.PerAgentDeviceLearner(stacked, obs_critic, PC.CFG)
    with pytest.raises(E):
        learner.DeviceLearner(shared_actor, obs_critic, LC.CFG, device_policy=ok)
    L = mk(device_policy=ok)
    with pytest.raises(ValueError, match="state_drones"):
        L.train_rollout(**{k: v for k, v in ro.items() if k not in ("state_drones", "next_state_last")})
    with pytest.raises(ValueError, match="state_drones"):
        L.train_rollout(**{**ro, "state_drones": ro["state_drones"][:, :2]})


class _Env:
    """The collector's env surface on the CPU: observations and state are functions of a step counter; an episode is 3 steps, so a collect of
    4 crosses a boundary."""
    max_episode_length = 3

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


def test_collector_needs_no_change_for_the_new_policy(cases):
    state, _ = cases[False]
    pol = PC.make_policy(state, seed=3)
    st = collector.DeviceCollector(_Env(), pol, T).collect()
    kw = st.learner_kwargs()
    assert kw["state_drones"].shape == (N, T, A, D) and kw["next_state_last"].shape == (N, A, D) and bool(kw["done"].any())
    hand, ref = _Env(), PC.make_policy(state, seed=3)
    cur = hand.reset()
    for t in range(T):
        obs, sd = cur[("agents", "observation")], cur[("agents", "state")]["state_drones"]
        out = ref.forward(obs["state_self"], obs["state_others"], obs["cylinders"], sd)
        assert torch.equal(kw["state_drones"][:, t], sd) and torch.equal(kw["state_value"][:, t], out.value), t
        assert torch.equal(kw["action"][:, t], out.action) and torch.equal(kw["log_probs"][:, t], out.log_prob), t
        cur = hand.step(None)["next"]
    assert torch.equal(kw["next_state_last"], cur[("agents", "state")]["state_drones"])
    a = PC.clone_state(state)
    info = PC.make_learner(a, seed=1).train_rollout(**kw)
    assert np.isfinite(list(info.values())).all()
