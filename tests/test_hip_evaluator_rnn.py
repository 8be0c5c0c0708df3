"""Recurrent device evaluation on the GPU: hns_policy_act_rnn (through RecurrentDevicePolicy.act_step and through the C ABI), DeviceEvaluator
with a recurrent policy, and the recurrent example's --eval flag.

hns_policy_act_rnn: `action` and the actor's state are bit for bit hns_policy_forward_rnn's with HNS_POLICY_DETERMINISTIC at every step of a
chain in which act_step's own state feeds its next call (flags at steps 0 and 3; test_hip_evaluator.py's shapes around the 32-row tile and
the shape with every limit at its maximum; contiguous and sliced observations; the state out of place and in place).  The call writes
nothing but `action` and `actor_h_out`, reads neither critic half of the two packed images, nor critic_h_in, nor a flagged env's h_in, nor
the call counter, and a row does not depend on the other rows.  DeviceEvaluator: `stats` and the means equal a hand loop that carries both
states through forward(deterministic=True) and the reference's take_first_episode over that loop's stacked statistics, and differ from a
loop that drops the state after every step; an evaluation between two collect()s of a recurrent collector leaves the second rollout bit for
bit what it is without it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_cases as EC
import eval_rnn_cases as ERC
import learner_cases as LC
import policy_rnn_reference as RR
from hns_amd import abi, collector, evaluator
from hns_amd import policy as P
from test_hip_evaluator import ACT_SHAPES, _make_env, _obs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
# (A, K, D, E): test_hip_evaluator.py's, and every limit at its maximum (21 rows of 7 agents)
SHAPES = ACT_SHAPES + [(7, 16, 96, 3)]


def _policy(A, D, seed):
    actor, critic = RR.random_net(D, A, seed)
    t = lambda p: {k: torch.as_tensor(np.asarray(v)).to(DEV) for k, v in p.items()}          # noqa: E731
    return P.RecurrentDevicePolicy(t(actor), t(critic), seed=seed)


def _states(E, A, seed):
    return tuple(torch.from_numpy(h).to(DEV) for h in RR.random_states(E, A, seed))


# ---------------------------------------------------------------------------------------------------------------------------------------
# hns_policy_act_rnn
@pytest.mark.parametrize("sliced", [False, True], ids=["contiguous", "sliced"])
@pytest.mark.parametrize("shape", SHAPES, ids=["a%dk%dd%de%d" % s for s in SHAPES])
def test_act_step_is_the_deterministic_forwards_actor_half_bit_for_bit_along_a_chain(shape, sliced):
    A, K, D, E = shape
    pol = _policy(A, D, 900 + 10 * A + K + D)
    flags = ERC.chain_flags(E, 50 + E)
    h0, hc = _states(E, A, 60 + E)
    ha, hw, hi = h0, h0, h0.clone()                              # act_step's chain, the forward's chain, act_step's in place
    out = torch.full((E, A, 4), 7.0, device=DEV)
    counter = pol.counter.clone()
    for t in range(ERC.STEPS):
        x, f = _obs(E, A, K, D, 17 + E + 100 * t, sliced), torch.from_numpy(flags[t]).to(DEV)
        want = pol.forward(*x, actor_state=hw, critic_state=hc, is_init=f, deterministic=True)
        action, ha = pol.act_step(*x, state=ha, is_init=f)
        assert action.shape == (E, A, 4) and ha.shape == (E, A, 128)
        for got in (action, ha):
            assert torch.isfinite(got).all() and float(got.abs().max()) > 0
        assert LC.bits_equal(action, want.action) and LC.bits_equal(ha, want.actor_state), t
        got = pol.act_step(*x, state=hi, is_init=f, out=out, out_state=hi)
        assert got[0] is out and got[1] is hi and LC.bits_equal(out, want.action) and LC.bits_equal(hi, want.actor_state), t
        hw, hc = want.actor_state, want.critic_state
    assert torch.equal(pol.counter, counter)


@pytest.mark.parametrize("shape", [(1, 5, 35, 33), (3, 5, 35, 11)], ids=["a1", "a3"])
def test_act_rnn_writes_only_the_action_and_the_actor_state_and_reads_nothing_of_the_critic(shape):
    A, K, D, E = shape
    rows = E * A
    pol = _policy(A, D, 5)
    x = _obs(E, A, K, D, 6)
    h, hc = _states(E, A, 7)
    flags = torch.zeros(E, dtype=torch.bool, device=DEV)
    flags[[1, 4, E - 1]] = True
    want = pol.forward(*x, actor_state=h, critic_state=hc, is_init=flags, deterministic=True)
    want_action, want_state = want.action.clone(), want.actor_state.clone()
    counter = pol.counter.clone()
    # rows do not depend on the other rows of the call: one env alone (flagged and not) gives the rows it has in the full call
    for e in (0, 1, E - 2):
        one = pol.act_step(*(t[e:e + 1] if t is not None else None for t in x), state=h[e:e + 1].contiguous(), is_init=flags[e:e + 1])
        assert LC.bits_equal(one[0], want_action[e:e + 1]) and LC.bits_equal(one[1], want_state[e:e + 1]), e
    G = 64                                                       # guard words behind every output
    action, h_out = torch.full((rows * 4 + G,), -77.0, device=DEV), torch.full((rows * 128 + G,), -78.0, device=DEV)
    others = {k: torch.full((n + G,), v, device=DEV) for k, n, v in (("log_prob", rows, 11.0), ("value", rows, 12.0), ("loc", rows * 4, 13.0))}
    critic_out = torch.full((rows * 128 + G,), 14.0, device=DEV)
    # what must never be read: NaN in the critic's state, in the state of the flagged envs, in the critic halves of BOTH packed images
    h_in = h.clone()
    h_in[flags] = float("nan")
    critic_in = torch.full((rows * 128,), float("nan"), device=DEV)
    for img in (pol.packed.view(torch.float32), pol.rnn_packed.view(torch.float32)):
        img[img.numel() // 2:] = float("nan")
    xs, xo, xc, io = pol._io(x[0].squeeze(2), x[1], x[2])
    io.action = action.data_ptr()
    for k, t in others.items():
        setattr(io, k, t.data_ptr())
    rio = abi.HnsPolicyRnnIo()
    rio.actor_h_in, rio.actor_h_out, rio.critic_h_in, rio.critic_h_out = h_in.data_ptr(), h_out.data_ptr(), critic_in.data_ptr(), critic_out.data_ptr()
    rio.is_init = flags.view(torch.uint8).data_ptr()
    lib = abi.load_library()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    abi.check(lib.hns_policy_act_rnn(pol.packed.data_ptr(), pol.rnn_packed.data_ptr(), D, E, A, K, C.byref(io), C.byref(rio), st), "hns_policy_act_rnn")
    torch.cuda.synchronize()
    assert LC.bits_equal(action[:rows * 4].view(E, A, 4), want_action) and LC.bits_equal(h_out[:rows * 128].view(E, A, 128), want_state)
    assert bool((action[rows * 4:] == -77.0).all()) and bool((h_out[rows * 128:] == -78.0).all())
    for (k, t), v in zip(others.items(), (11.0, 12.0, 13.0)):
        assert bool((t == v).all()), f"{k} was written"
    assert bool((critic_out == 14.0).all()) and bool(torch.isnan(critic_in).all()) and bool(torch.isnan(h_in[flags]).all())
    assert torch.equal(pol.counter, counter)
    # NULL for everything the call ignores, the same inputs, the same bits; and through the class, in place
    for k in others:
        setattr(io, k, None)
    rio.critic_h_in = rio.critic_h_out = None
    again = torch.full_like(h_out, -78.0)
    rio.actor_h_out = again.data_ptr()
    abi.check(lib.hns_policy_act_rnn(pol.packed.data_ptr(), pol.rnn_packed.data_ptr(), D, E, A, K, C.byref(io), C.byref(rio), st), "hns_policy_act_rnn")
    torch.cuda.synchronize()
    assert LC.bits_equal(again, h_out) and LC.bits_equal(action[:rows * 4].view(E, A, 4), want_action)
    got = pol.act_step(xs, xo, xc, state=h_in, is_init=flags, out_state=h_in)
    assert LC.bits_equal(got[0], want_action) and got[1] is h_in and LC.bits_equal(h_in, want_state) and torch.equal(pol.counter, counter)


# ---------------------------------------------------------------------------------------------------------------------------------------
# DeviceEvaluator against the hand loops
def _env_policy(env, seed):
    D = abi.self_dim(env.num_targets) + (3 * env.tp_future_step * env.num_targets if env.use_TP_net else 0)
    actor, critic = P.random_parameters(D, env.num_agents, seed=seed)
    actor.update(P.random_rnn_parameters(seed + 1))
    critic.update(P.random_rnn_parameters(seed + 2))
    actor["act_dist.fc_mean.weight"] = actor["act_dist.fc_mean.weight"] * 30.0    # actions of order 0.3: the drones move
    return P.RecurrentDevicePolicy(actor, critic, device=env.device, seed=seed)


@pytest.mark.parametrize("use_tp", [0, 1], ids=["plain", "predictor"])
def test_evaluate_equals_the_stateful_hand_loop_and_not_the_stateless_one(use_tp):
    N, L = 64, 6
    task = {"num_agents": 3, "env": {"num_envs": N, "max_episode_length": L}}
    env, hand, amnesic = (_make_env(task, use_tp) for _ in range(3))
    try:
        pol = _env_policy(env, 8)
        counter = pol.counter.clone()
        ev = evaluator.DeviceEvaluator(env, pol)
        info = ev.evaluate(seed=3)
        assert (ev.steps, ev.done_reads, ev.launches) == (L, 1, 1) and torch.equal(pol.counter, counter)
        stacked = {k: [] for k in (*abi.STAT_NAMES, "done")}
        ERC.hand_loop(hand, pol, 3, hand.rand_step_input, stateful=True, stacked=stacked)
        ERC.hand_loop(amnesic, pol, 3, amnesic.rand_step_input, stateful=False)
        done = torch.stack(stacked["done"], dim=1)                                # [N, L, 1]
        assert bool(done[:, -1].all()) and not bool(done[:, :-1].any())           # pure truncation
        first_done = torch.argmax(done.long(), dim=1)
        assert set(info) == {"eval/stats." + k for k in abi.STAT_NAMES} == {"eval/stats." + k for k in ev.stats}
        moved = differ = 0
        for k in abi.STAT_NAMES:
            traj = torch.stack(stacked[k], dim=1)                                 # [N, L, 1]
            first = torch.take_along_dim(traj, first_done.reshape(first_done.shape + (1,) * (traj.ndim - 2)), dim=1).reshape(-1)
            assert ev.stats[k].shape == (N,) and LC.bits_equal(ev.stats[k], hand.stats[k].reshape(-1)), k
            assert LC.bits_equal(ev.stats[k], first), k
            want, _, _ = evaluator.stat_means([hand.stats[k]], None)              # the kernel's order on the host: the same bits
            assert np.array_equal(np.array([info["eval/stats." + k]], np.float32), want, equal_nan=True), k
            EC.check_mean(info["eval/stats." + k], ev.stats[k].cpu().numpy(), None, k)
            moved += bool((traj[:, -1] != traj[:, 0]).any())
            differ += not LC.bits_equal(ev.stats[k], amnesic.stats[k].reshape(-1))
        assert moved >= 3                                                         # the statistics are not all constants of the episode
        assert differ >= 1                                                        # a loop that zeroes the state every step is another run
        again = ev.evaluate(seed=3)
        a, b = (np.array([d["eval/stats." + k] for k in abi.STAT_NAMES], np.float32) for d in (info, again))
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
        other = ev.evaluate(seed=4)
        assert any(other["eval/stats." + k] != info["eval/stats." + k] for k in abi.STAT_NAMES)   # ... and the seed is what seeds it
        assert (ev.steps, ev.done_reads, ev.launches) == (3 * L, 3, 3) and torch.equal(pol.counter, counter)
    finally:
        for e in (env, hand, amnesic):
            e.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# training is undisturbed
def _collecting_side(with_eval):
    """Two collect()s of a recurrent collector (sampling: the call counter moves), optionally with an evaluation on a separate 32-env env
    between them: clones of the second rollout's storage, and the counter."""
    N, T, A = 64, 8, 3
    env = _make_env({"num_agents": A, "env": {"num_envs": N, "max_episode_length": 12}}, 1, seed=3)
    eval_env = _make_env({"num_agents": A, "env": {"num_envs": 32, "max_episode_length": 10}}, 1, seed=9)
    try:
        pol = _env_policy(env, 4)
        col = collector.DeviceCollector(env, pol, T, rnn_seq_len=4)
        ev = evaluator.DeviceEvaluator(eval_env, pol, tp_net=env.TP)
        torch.manual_seed(77)                                    # both sides start the global generators (CPU and device) from one state
        col.collect()
        if with_eval:
            counter, states = pol.counter.clone(), tuple(s.clone() for s in col._states)
            res = ev.evaluate(seed=0)
            assert len(res) == abi.HNS_NUM_STATS and ev.steps == 10
            assert torch.equal(pol.counter, counter) and int(counter) == T       # the evaluation draws no noise
            assert all(LC.bits_equal(a, b) for a, b in zip(col._states, states))
        st = col.collect()
        assert bool(st.data["done"].any())                       # an episode boundary inside the second rollout
        return {part: {k: v.clone() for k, v in getattr(st, part).items()} for part in ("data", "segments", "last")}, int(pol.counter)
    finally:
        env.close()
        eval_env.close()


def test_an_evaluation_between_two_collects_leaves_the_second_rollout_bit_for_bit():
    plain, c0 = _collecting_side(False)
    mixed, c1 = _collecting_side(True)
    assert c0 == c1 == 16
    for part in ("data", "segments", "last"):
        assert set(plain[part]) == set(mixed[part])
        for k, v in plain[part].items():
            assert LC.bits_equal(mixed[part][k], v), (part, k)
    assert {"is_init", "action"} <= set(plain["data"]) and set(plain["segments"]) == set(collector.RNN_STATES)


def test_an_evaluation_on_the_training_env_puts_it_back_and_the_collector_restarts_with_every_flag_set():
    N, T, L = 64, 8, 6
    env = _make_env({"num_agents": 3, "env": {"num_envs": N, "max_episode_length": L}}, 1, seed=3)
    try:
        pol = _env_policy(env, 8)
        col = collector.DeviceCollector(env, pol, T, rnn_seq_len=4)
        col.collect()
        env.eval()                                               # (whatever the flag is, it comes back)
        before = (env.training, env.seed, env.reset_epoch)
        assert before[0] is False and before[1] == 3
        cpu_rng, dev_rng = torch.get_rng_state().clone(), torch.cuda.get_rng_state(env.device).clone()
        counter = pol.counter.clone()
        calls = []
        reset = env.reset
        env.reset = lambda td=None, **kw: (calls.append(td is None), reset(td, **kw))[1]
        evaluator.DeviceEvaluator(env, pol, collector=col).evaluate(seed=5)
        assert (env.training, env.seed, env.reset_epoch) == before and torch.equal(pol.counter, counter)
        assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(env.device), dev_rng)
        assert calls == [True]
        env.train()
        st = col.collect()
        assert calls[1] is True and calls.count(True) == 2       # the collector's next collect() starts from ONE full reset
        assert env.reset_epoch > before[2]
        assert bool(st.data["is_init"][:, 0].all()) and not bool(st.data["is_init"][:, 1:L].any())
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the example script
def test_the_recurrent_example_evaluates():
    script = os.path.join(ROOT, "examples", "recurrent_policy.py")
    run = subprocess.run([sys.executable, script, "--envs", "64", "--steps", "16", "--updates", "1", "--eval"], capture_output=True, text=True,
                         timeout=240)
    assert run.returncode == 0, run.stdout + run.stderr
    for k in abi.STAT_NAMES:
        assert run.stdout.count("eval/stats." + k + " = ") == 1, k
    assert "rollout 1 update 0" in run.stdout
